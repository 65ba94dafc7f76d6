"""Child of tests/test_tri_placement_gpu.py: `python tests/placement_child.py <step> <out.npy>` renders step <step> of the
drifting scene as the FIRST call of a fresh process -- no placement exists yet, so the call goes through the exact path
(set-up -> scan -> scatter) -- and saves [colour | depth] for the parent to compare bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np
import torch as th

from dmesh_renderer_amd.scenes import c_args


if __name__ == "__main__":
    from test_tri_placement_gpu import DRIFT, drift_scene
    from dmesh_renderer_amd import _C
    step, path = int(sys.argv[1]), sys.argv[2]
    B, H, W = DRIFT
    redo0 = _C.redo_count()
    out = _C.render_tris(*c_args(drift_scene(step), th.device("cuda:0")), H, W)
    th.cuda.synchronize()
    assert _C.redo_count() == redo0
    np.save(path, np.concatenate([out[1].cpu().numpy().reshape(-1), out[2].cpu().numpy().reshape(-1)]))
    print("placement child ok", out[0])
