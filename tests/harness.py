"""Test-only helpers (a plain module, imported like util.py): the one launcher of child processes (two gloo ranks of
tests/sharded_child.py; tests/fallback_child.py on the ablation build), the graph capture ritual, the
clone-call-backpropagate step of a Module, and tri calls through the C ABI with a guarded allocator."""
import ctypes as C
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


class GuardedTriCalls:
    """dmr_tri_forward / dmr_tri_backward through the C ABI with an allocator of its own: every buffer the library asks for is
    followed by GUARD bytes of 0xA5, checked after every call -- a store behind a scratch buffer fails the call's test.
    `lib` is the library with the ABI's signatures bound (dmr_overflowed, dmr_redo_count, ...)."""
    GUARD = 4096

    def __init__(self, dev):
        from dmesh_renderer_amd import _C
        import capi_ctypes as capi
        self.capi, self.dev = capi, dev
        self.lib = C.CDLL(_C.library_path())
        for name, (restype, argtypes) in capi.EXPORTS.items():
            getattr(self.lib, name).restype = restype
            getattr(self.lib, name).argtypes = argtypes
        self.held = []      # (tensor with its guard, bytes asked for, which) of the call in hand
        self.buffers = {}   # the last forward's scratch by DMR_BUF_*, without the guards

        def alloc(_ctx, which, nbytes):
            t = th.full((int(nbytes) + self.GUARD,), 0xA5, dtype=th.uint8, device=dev)
            self.held.append((t, int(nbytes), int(which)))
            return t.data_ptr()

        self.alloc_fn = capi.ALLOC_FN(alloc)

    def _scene(self, d, B, H, W, flags):
        from util import c_args
        a = [x.contiguous() for x in c_args(d, self.dev)]
        a[2] = a[2].to(th.int32).contiguous()
        sc = self.capi.Scene(B=B, P=a[1].shape[0], F=a[2].shape[0], T=0, W=W, H=H, background=a[0].data_ptr(), verts=a[1].data_ptr(),
                             faces=a[2].data_ptr(), verts_color=a[3].data_ptr(), faces_opacity=a[4].data_ptr(), mv_mats=a[5].data_ptr(),
                             proj_mats=a[6].data_ptr(), inv_mv_mats=a[7].data_ptr(), inv_proj_mats=a[8].data_ptr(),
                             verts_depth=a[9].data_ptr(), faces_intense=a[10].data_ptr(), tets=None, face_tets=None, tet_faces=None,
                             ray_random_seed=0, row_begin=0, row_end=0, mats_transposed=0, flags=flags)
        return sc, a

    def _guards_intact(self):
        for t, nbytes, _ in self.held:
            assert bool((t[nbytes:] == 0xA5).all()), "guard words behind a scratch buffer were overwritten"

    def forward(self, d, B, H, W, flags):
        """-> (the R the call returns, colour, depth, the call's tensor arguments); flags: DMR_FLAG_ASYNC = 1"""
        sc, a = self._scene(d, B, H, W, flags)
        color = th.empty(B, 3, H, W, device=self.dev)
        depth = th.empty(B, 1, H, W, device=self.dev)
        R = C.c_int(0)
        del self.held[:]
        rc = self.lib.dmr_tri_forward(C.byref(sc), color.data_ptr(), depth.data_ptr(), self.alloc_fn, None, None, C.byref(R))
        th.cuda.synchronize()
        assert rc == 0, self.lib.dmr_last_error()
        self._guards_intact()
        self.buffers = {which: t[:nbytes] for t, nbytes, which in self.held}
        return R.value, color, depth, a

    def backward(self, d, B, H, W, flags, R, gc, gd):
        """The backward of the last forward (same scene): -> [dL_dverts, dL_dvcolor, dL_dfopacity, dL_dvdepth, dL_dfintense]"""
        sc, a = self._scene(d, B, H, W, flags)
        P, F = a[1].shape[0], a[2].shape[0]
        gc, gd = gc.to(self.dev).contiguous(), gd.to(self.dev).contiguous()
        out = [th.full(s, float("nan"), device=self.dev) for s in ((P, 3), (P, 3), (F,), (B, P), (B, F))]
        capi = self.capi
        buf = [self.buffers[w].data_ptr() for w in (capi.BUF_POINT, capi.BUF_FACE, capi.BUF_BINNING, capi.BUF_IMAGE)]
        del self.held[:]
        rc = self.lib.dmr_tri_backward(C.byref(sc), gc.data_ptr(), gd.data_ptr(), int(R), *buf, *[o.data_ptr() for o in out],
                                       self.alloc_fn, None, None)
        th.cuda.synchronize()
        assert rc == 0, self.lib.dmr_last_error()
        self._guards_intact()
        return out
