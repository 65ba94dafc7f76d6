"""Test-only helpers (a plain module, imported like util.py): the one launcher of child processes (two gloo ranks of
tests/sharded_child.py; tests/fallback_child.py on the ablation build), the graph capture ritual, and the
clone-call-backpropagate step of a Module."""
import os
import signal
import socket
import subprocess
import sys
import tempfile

import torch as th

HERE = os.path.dirname(os.path.abspath(__file__))

TRI_ARGS = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
TET_ARGS = TRI_ARGS + ("tets", "face_tets", "tet_faces")


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_child(cmd, ok_line, timeout, grace=5, **env):
    """Run `cmd` once, in a session of its own, and assert that it exits with status 0 and prints `ok_line`.  On a
    time-out the whole process group is ended (TERM, `grace` seconds, KILL) and waited for, so that no descendant stays
    behind with the GPU open or a port bound, and the test fails; there is no second attempt."""
    with tempfile.TemporaryFile("w+") as out, tempfile.TemporaryFile("w+") as err:  # files: no pipe a descendant could hold open
        p = subprocess.Popen(cmd, env=dict(os.environ, **env), stdout=out, stderr=err, start_new_session=True)
        try:
            code = p.wait(timeout)
        except BaseException as e:  # the time-out, or the test run itself being interrupted
            for sig, wait in ((signal.SIGTERM, grace), (signal.SIGKILL, None)):
                try:
                    os.killpg(p.pid, sig)
                    p.wait(wait)
                except (ProcessLookupError, subprocess.TimeoutExpired):
                    pass
            if not isinstance(e, subprocess.TimeoutExpired):
                raise
            code = None
        out.seek(0); err.seek(0)
        stdout = out.read()
        tails = stdout[-2000:] + err.read()[-4000:]
    assert code is not None, f"timed out after {timeout} s; its process group was ended\n" + tails
    assert code == 0 and ok_line in stdout, tails


def run_ranks(case, ok_line, nproc=2, timeout=400):
    """`nproc` gloo ranks of tests/sharded_child.py <case> on the one GPU, on a port that is free now."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(HERE, "sharded_child.py"), case]
    _run_child(cmd, ok_line, timeout, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")


def run_ablation_child(case, ok_line, ablate="2048", timeout=300):
    """tests/fallback_child.py <case> on the ablation build of the library (build.py --ablation; the product library has
    no such switch and ignores the variable): 2048 refuses rows with an odd id a table slot."""
    from dmesh_renderer_amd import build
    lib = build.build(ablation=True)  # prebuilt by __graft_entry__.build(); compiled here only if missing or stale
    _run_child([sys.executable, os.path.join(HERE, "fallback_child.py"), case], ok_line, timeout, DMR_ABLATE=ablate, DMR_LIBRARY=lib)


def capture_replay(step, warmup=2, reset=None):
    """Capture `step()` into a HIP graph -> (graph, what the captured step returned, clones of what the last eager step
    returned, or None).  The order matters: the warm-up on a side stream makes default (waiting) calls, which leave the
    size estimates the captured calls need; `reset()` (say, clearing .grad) runs between warm-up and capture; the sticky
    overflow flag is cleared by a read before the capture, and read again by replay()."""
    from dmesh_renderer_amd import _C
    side = th.cuda.Stream()
    side.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(side):
        for _ in range(warmup):
            eager = step()
            eager = None if eager is None else [x.detach().clone() for x in eager]
    th.cuda.current_stream().wait_stream(side)
    th.cuda.synchronize()
    if reset is not None:
        reset()
    _C.overflowed()
    graph = th.cuda.CUDAGraph()
    with th.cuda.graph(graph):
        captured = step()
    return graph, captured, eager


def replay(graph, times=1):
    """Replay, wait, and assert that no replayed call outgrew the capacity it was captured with."""
    from dmesh_renderer_amd import _C
    for _ in range(times):
        graph.replay()
    th.cuda.synchronize()
    assert not _C.overflowed(), "the replayed scene outgrew the captured capacity"


def module_step(renderer, t, grad_names, upstream):
    """Clone the leaves `grad_names` of the scene `t`, call a tri or tet Module (tet: `t` has "tets") with its positional
    arguments, backpropagate `upstream` into the first len(upstream) differentiable outputs
    -> (outputs detached, {name: grad})."""
    leaves = {k: t[k].clone().requires_grad_(True) for k in grad_names}
    out = renderer(*(leaves[k] if k in leaves else t[k] for k in (TET_ARGS if "tets" in t else TRI_ARGS)))
    th.autograd.backward([o for o in out if o.requires_grad][:len(upstream)], list(upstream))
    return [o.detach() for o in out], {k: leaves[k].grad for k in grad_names}
