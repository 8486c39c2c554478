"""gen_linemod_golden.py -- golden vectors for the dataset reader (neural_sim_nerf_amd/data.py: load_LINEMOD_data) from the
reference's own LL:97-163, run on the seeded synthetic dataset that tests/test_data_readers.py writes (_make_dataset).

Two shims, both outside the arithmetic under test: imageio and cv2 are replaced by stand-in modules whose imread is this
package's PNG decoder, and `pose_spherical` by the reference's own `pose_spherical_nograd` -- the published call
`pose_spherical(angle, -30.0, 1.01)` raises on a python float (LL:63); whether it still does is recorded too.

Run:  python oracle/gen_linemod_golden.py <the reference checkout's optimization/ directory>
Writes tests/golden/g27_linemod_reader.npz.  Test infrastructure only.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g27_linemod_reader.npz")


def main(ref_dir):
    sys.path.insert(0, ROOT)
    from neural_sim_nerf_amd import png
    spec = importlib.util.spec_from_file_location("_test_data_readers", os.path.join(ROOT, "tests", "test_data_readers.py"))
    tdr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tdr)
    for m in ("imageio", "cv2"):
        sys.modules[m] = types.ModuleType(m)
    sys.modules["imageio"].imread = png.imread
    sys.path.insert(0, ref_dir)
    import utils.load_LINEMOD_noscale as LL
    with tempfile.TemporaryDirectory() as d:
        tdr._make_dataset(d)
        try:
            LL.load_LINEMOD_data(d, False, 2)
            raised = False
        except AttributeError:
            raised = True
        LL.pose_spherical = LL.pose_spherical_nograd
        imgs, poses, render_poses, hwf, K, i_split, near, far = LL.load_LINEMOD_data(d, False, 2)
    np.savez_compressed(OUT, imgs=imgs, poses=poses, render_poses=render_poses.numpy(), hwf=np.asarray(hwf, np.float64),
                        K=np.asarray(K, np.float64), i_train=i_split[0], i_val=i_split[1], i_test=i_split[2],
                        near=np.float64(near), far=np.float64(far), pose_spherical_raises=np.bool_(raised))
    print("wrote", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
