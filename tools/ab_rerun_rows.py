"""A/B of the layered renderer's two re-run units on f16x2 -- WideModel(rerun="pass"), the default, against rerun="rows" (DESIGN.md 8
"Row-granular re-run") -- with the parent commit's tree on either side as the yardstick of the run-to-run spread:

    python tools/ab_rerun_rows.py --parent DIR [--hw 400] [--steps 7] [--workloads clean,inf,d8w64,range] [--out FILE]

DIR is a checkout of the parent commit with its libnsr.so built.  Four processes in turn: the parent's tree, this tree ("pass", then
"rows", in ONE process on the same rays), the parent's tree again.  A worker process imports the package of the tree it is handed and
nothing else of the other one; a parent worker builds its handles without the `rerun` keyword.  Per workload and mode: the device
time of one 400x400 view (nsrw_last_ms: events around the launches of a call), forward and forward + rgb gradient, over `steps` calls
behind one warm-up call -- median [min, max] -- and the handle's range counters.  "pass" against the parent is the price of the
change on the default path and has to sit inside parent-against-parent; "rows" against "pass" is reported as it is.

Workloads (tools/bench_wide.py's networks and view):
  clean   8 x 256 at 64 + 128, nothing leaves fp16's range: the mode's fixed cost (bit stores, two list launches, the wider tally)
  inf     the same view with one ray of infinite direction in every chunk of the call (placed by the chunk size the library uses, and
          checked: both forward passes of every chunk re-run): "pass" re-runs those passes whole
  d8w64   8 x 64 at 64 + 128, which re-runs a quarter of its passes on its own values: the share of rows that is behind it
  range   8 x 128 whose coarse network leaves the range on every point (bench_wide's d8w128range): every row flagged
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"clean": "ycbv", "inf": "ycbv", "d8w64": "d8w64", "range": "d8w128range"}


def worker(tree, modes, a):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    import numpy as np
    import torch
    from bench_wide import CASES, RANGE_CASES, net_sd
    from neural_sim_nerf_amd import synthetic as S
    from neural_sim_nerf_amd.wide import WideModel
    K = S.scaled_K(400.0 / a.hw)
    pose = S.sweep_poses(1, seed=0)[0]
    for wl in a.workloads.split(","):
        D, W, L, Lv, skips, ns, ni = CASES[WORKLOADS[wl]]
        sd = net_sd(D, W, L, Lv, skips, 1)
        sd_c = sd
        if WORKLOADS[wl] in RANGE_CASES:
            sd_c = {k: v.copy() for k, v in sd.items()}
            sd_c["pts_linears.1.bias"][5] += 7.0e4
        for mode in modes:
            kw = {} if mode == "parent" else {"rerun": mode}
            m = WideModel(sd_c, sd, n_samples=ns, n_importance=ni, mlp="f16x2", **kw)
            n = a.hw * a.hw
            ro, rd = m.get_rays(a.hw, a.hw, K, torch.tensor(pose[:3, :4]))
            ro, rd = ro.reshape(-1, 3).clone(), rd.reshape(-1, 3).clone()
            torch.manual_seed(0)
            cot = torch.randn(n, 3, device=m.device)
            res = {"workload": wl, "mode": mode, "network": "%d x %d at %d + %d" % (D, W, ns, ni), "rays": n}
            for what in ("forward", "forward+gradient"):
                call = (lambda: m.render_rays(ro, rd, S.YCBV_NEAR, S.YCBV_FAR)) if what == "forward" else \
                       (lambda: m.render_rays_vjp(ro, rd, S.YCBV_NEAR, S.YCBV_FAR, cot))
                call()                                               # warm-up; and how many chunks this call is cut into
                chunks = m.last_kernel_ms()[1]
                if wl == "inf":
                    # one infinite ray in every chunk.  The library cuts a call into chunks of R rays, the LARGEST multiple of 64 whose
                    # chunk fits the workspace it was handed (every chunk full but the last): R from the same two figures
                    grad = 0 if what == "forward" else 1
                    lo, hi = 64, (n + 63) // 64 * 64
                    if m._need(hi, grad) <= m.workspace_bytes:
                        lo = hi
                    while hi - lo > 64:
                        mid = (lo + hi) // 2 // 64 * 64
                        lo, hi = (mid, hi) if m._need(mid, grad) <= m.workspace_bytes else (lo, mid)
                    R = lo
                    if -(-n // R) != chunks:
                        sys.exit("inf: %d rays in chunks of %d are not the %d chunks the call ran" % (n, R, chunks))
                    bad = [min(n - 1, i * R + 7) for i in range(chunks)]
                    saved = rd[bad, 0].clone()
                    rd[bad, 0] = float("inf")
                    res[what + " infinite rays"] = len(bad)
                    res[what + " chunk rays"] = R
                    call()
                before = m.range_status()
                ms = []
                for _ in range(a.steps):
                    call()
                    ms.append(m.last_kernel_ms()[0])
                after = m.range_status()
                res[what] = {"ms": round(float(np.median(ms)), 2), "min": round(min(ms), 2), "max": round(max(ms), 2), "chunks": chunks}
                res[what].update({k: (after[k] - before[k]) // a.steps for k in ("passes", "passes_rerun", "rows", "rows_rerun") if k in after})
                if wl == "inf":
                    rd[bad, 0] = saved
                    # the coarse and the fine forward of EVERY chunk hold infinite points: both leave the range in every chunk
                    if res[what]["passes_rerun"] < 2 * chunks:
                        sys.exit("inf: %d passes re-run in %d chunks: some chunk holds no infinite ray" % (res[what]["passes_rerun"], chunks))
            print("RESULT " + json.dumps(res), flush=True)
            m.close()
            del m
            torch.cuda.empty_cache()


def run(tree, modes, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--modes", ",".join(modes), "--hw", str(a.hw), "--steps", str(a.steps),
           "--workloads", a.workloads]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=900)
    if r.returncode != 0:
        sys.exit("worker on %s failed:\n%s" % (tree, r.stderr[-3000:]))
    return [json.loads(l[7:]) for l in r.stdout.splitlines() if l.startswith("RESULT ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--worker")
    ap.add_argument("--modes", default="pass,rows")
    ap.add_argument("--hw", type=int, default=400)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--workloads", default="clean,inf,d8w64,range")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.modes.split(","), a)
    if not a.parent:
        ap.error("--parent DIR")
    runs = [("parent (first)", run(a.parent, ["parent"], a)), ("this tree", run(HERE, ["pass", "rows"], a)), ("parent (again)", run(a.parent, ["parent"], a))]
    lines = ["layered renderer, f16x2, one %dx%d view, %d calls behind a warm-up: median ms [min, max] of the device time of a call" % (a.hw, a.hw, a.steps),
             "order of the processes: parent, this tree (pass then rows in one process), parent again", ""]
    for wl in a.workloads.split(","):
        rows = [(label if r["mode"] == "parent" else 'rerun="%s"' % r["mode"], r) for label, rs in runs for r in rs if r["workload"] == wl]
        lines.append("%s: %s" % (wl, rows[0][1]["network"]))
        for what in ("forward", "forward+gradient"):
            lines.append("  %s" % what + (" (%d infinite rays, one per chunk of %d rays)" % (rows[0][1][what + " infinite rays"], rows[0][1][what + " chunk rays"])
                                          if wl == "inf" else ""))
            for label, r in rows:
                t = r[what]
                share = ", rows re-run %d of %d (%.4f %%)" % (t["rows_rerun"], t["rows"], 100.0 * t["rows_rerun"] / max(1, t["rows"])) if t.get("rows") else ""
                lines.append("    %-16s %8.2f [%8.2f, %8.2f] ms  chunks %d  passes re-run %d of %d%s"
                             % (label, t["ms"], t["min"], t["max"], t["chunks"], t["passes_rerun"], t["passes"], share))
            p = [r[what]["ms"] for label, r in rows if label.startswith("parent")]
            ab = {r["mode"]: r[what]["ms"] for _, r in rows}
            lines.append("    parent against parent %+.2f %%; pass against the parents' mean %+.2f %%; rows against pass %+.2f %%"
                         % (100.0 * (p[1] / p[0] - 1), 100.0 * (ab["pass"] / (0.5 * (p[0] + p[1])) - 1), 100.0 * (ab["rows"] / ab["pass"] - 1)))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
