"""Test-only helpers (a plain module, imported like util.py): the one launcher of child processes (two gloo ranks of
tests/sharded_child.py; tests/fallback_child.py on the ablation build), the graph capture ritual, the
clone-call-backpropagate step of a Module, and the four entry points of the C ABI through ctypes with a guarded, poisoned
allocator (GuardedCalls; GuardedTriCalls: its default tri calls under their earlier names)."""
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


class _Result:
    """What one guarded call returned: attributes by name (see the four methods of GuardedCalls)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class GuardedCalls:
    """The four entry points of the C ABI (include/dmesh_renderer_amd.h) through ctypes, with an allocator and outputs of its own.

    Every buffer the library requests through `alloc`, and every tensor the caller owns (the images, the gradient outputs), is the
    body of a flat tensor [GUARD bytes of 0xA5 | body | GUARD bytes of 0xA5]; the body starts 256-byte aligned and the back guard
    starts at the first byte behind what was asked for.  Both guards of every buffer of a call -- and, after a backward, of the
    scratch its forward left -- are checked once the call has completed: a store one element in front of or behind a buffer fails
    the call's test.
      body_fill  the byte the scratch buffers (DMR_BUF_POINT .. DMR_BUF_WORK) hold when they are handed out (0xA5 or 0x00): a
                 kernel that relies on a zero it never wrote passes under one fill only;
      out_bits   the 32-bit pattern every OUTPUT holds before the call -- the caller-owned tensors and the output ids served
                 through `alloc` (gradients, camera gradients, fragment lists): NAN_BITS, a quiet NaN with a payload (as an
                 int32 a face id far outside any mesh), or 0;
      inputs     {DMR_BUF_*_FRAGMENT_FACES / _BARY_GRADS: tensor}, registered by the test before a backward: the callback hands
                 the library a guarded copy, filled before the call as the header requires;
      log        [(which, nbytes)] of the call in hand, in request order; served: {which: the body of the last request, uint8}.
    `lib` is the library with the ABI's signatures bound (dmr_overflowed, dmr_redo_count, ...)."""
    GUARD = 4096
    GUARD_BYTE = 0xA5
    NAN_BITS = 0x7FC5A5A5

    def __init__(self, dev, body_fill=0xA5, out_bits=NAN_BITS):
        from dmesh_renderer_amd import _C
        import capi_ctypes as capi
        self.capi, self.dev, self.body_fill, self.out_bits = capi, dev, int(body_fill), int(out_bits)
        self.lib = C.CDLL(_C.library_path())
        for name, (restype, argtypes) in capi.EXPORTS.items():
            getattr(self.lib, name).restype = restype
            getattr(self.lib, name).argtypes = argtypes
        self.held = []      # (flat tensor with both guards, bytes of the body, what it is) of the call in hand
        self.scratch = []   # ... of the last forward: checked again after its backward
        self.buffers = {}   # the last forward's scratch by DMR_BUF_*, without the guards
        self.log, self.served, self.inputs, self.errors = [], {}, {}, []

        def alloc(_ctx, which, nbytes):
            try:   # (an exception cannot cross the C frames: kept, and reported when the call has returned)
                which, nbytes = int(which), int(nbytes)
                self.log.append((which, nbytes))
                name = capi.BUF_NAMES[which]
                if which in capi.INPUT_BUFFERS:
                    src = self.inputs.get(which)
                    if src is None or src.numel() * src.element_size() < nbytes:
                        return None
                    body, ptr = self._guarded(nbytes, name)
                    body.copy_(src.contiguous().view(-1).view(th.uint8)[:nbytes])
                elif which in capi.OUTPUT_BUFFERS:
                    body, ptr = self._guarded(nbytes, name, self.out_bits)
                else:
                    body, ptr = self._guarded(nbytes, name)
                    body.fill_(self.body_fill)
                self.served[which] = body
                return ptr
            except BaseException as e:
                self.errors.append(e)
                return None

        self.alloc_fn = capi.ALLOC_FN(alloc)

    # ---- guarded memory ----------------------------------------------------------------------------------------------------
    def _guarded(self, nbytes, what, bits=None):
        """-> (the body, uint8 [nbytes], between its guards; its address).  bits: the 32-bit pattern it is filled with."""
        G = self.GUARD
        flat = th.full((2 * G + nbytes,), self.GUARD_BYTE, dtype=th.uint8, device=self.dev)
        ptr = flat.data_ptr() + G
        assert ptr % 256 == 0, "the body of a guarded buffer must start 256-byte aligned"
        body = flat[G:G + nbytes]
        if bits is not None and nbytes:
            assert nbytes % 4 == 0
            body.view(th.int32).fill_(bits - (1 << 32) if bits >= (1 << 31) else bits)
        self.held.append((flat, nbytes, what))
        return body, ptr

    def output(self, shape, what, dtype=th.float32):
        """A caller-owned tensor carved out of a guarded flat one, pre-filled with out_bits -> (tensor, its address or None)."""
        n = 1
        for s in shape:
            n *= int(s)
        body, ptr = self._guarded(4 * n, what, self.out_bits)
        return body.view(dtype).view(*shape), (ptr if n else None)

    def prefill(self, like):
        """A tensor of `like`'s shape and dtype (4-byte elements) that holds out_bits: what an untouched output must equal."""
        bits = self.out_bits - (1 << 32) if self.out_bits >= (1 << 31) else self.out_bits
        return th.full(like.shape, bits, dtype=th.int32, device=like.device).view(like.dtype)

    def check_guards(self, records=None):
        G = self.GUARD
        for flat, nbytes, what in (self.held if records is None else records):
            front = bool((flat[:G] == self.GUARD_BYTE).all())
            back = bool((flat[G + nbytes:] == self.GUARD_BYTE).all())
            assert front, f"the guard in front of {what} ({nbytes} bytes) was overwritten"
            assert back, f"the guard behind {what} ({nbytes} bytes) was overwritten"

    # ---- the call ----------------------------------------------------------------------------------------------------------
    def scene(self, d, H, W, flags=0, rows=(0, 0), mats_transposed=0, seed=0, tet=False):
        """-> (dmr_scene, the call's tensor arguments in contract layout (what _C.export takes), everything to keep alive).
        Bit i of mats_transposed: matrix i (mv, proj, inv_mv, inv_proj) is stored with its 4x4 blocks transposed."""
        from util import c_args
        a = [x.contiguous() for x in c_args(d, self.dev, tet=tet)]
        a[2] = a[2].to(th.int32).contiguous()
        mats = [a[5 + i].transpose(1, 2).contiguous() if (mats_transposed >> i) & 1 else a[5 + i] for i in range(4)]
        p = lambda t: t.data_ptr() if t.numel() else None
        topo = dict(tets=p(a[11]), face_tets=p(a[12]), tet_faces=p(a[13])) if tet else dict(tets=None, face_tets=None, tet_faces=None)
        sc = self.capi.Scene(B=a[5].shape[0], P=a[1].shape[0], F=a[2].shape[0], T=a[11].shape[0] if tet else 0, W=W, H=H,
                             background=p(a[0]), verts=p(a[1]), faces=p(a[2]), verts_color=p(a[3]), faces_opacity=p(a[4]),
                             mv_mats=p(mats[0]), proj_mats=p(mats[1]), inv_mv_mats=p(mats[2]), inv_proj_mats=p(mats[3]),
                             verts_depth=p(a[9]), faces_intense=p(a[10]), ray_random_seed=seed, row_begin=rows[0], row_end=rows[1],
                             mats_transposed=mats_transposed, flags=flags, **topo)
        return sc, a, (a, mats)

    def _begin(self):
        self.held, self.log, self.served, self.errors = [], [], {}, []

    def _end(self, rc, forward):
        th.cuda.synchronize()
        if self.errors:
            raise self.errors[0]
        assert rc == 0, self.lib.dmr_last_error()
        self.check_guards()
        if forward:
            self.scratch = list(self.held)
            self.buffers = {w: self.served[w] for w in range(self.capi.BUF_WORK) if w in self.served}
        else:
            self.check_guards(self.scratch)

    def _scratch_ptrs(self):
        capi = self.capi
        return [self.buffers[w].data_ptr() if w in self.buffers and self.buffers[w].numel() else None
                for w in (capi.BUF_POINT, capi.BUF_FACE, capi.BUF_BINNING, capi.BUF_IMAGE)]

    def _upstream(self, gc, gd):
        return gc.to(self.dev).contiguous(), gd.to(self.dev).contiguous()

    def tri_forward(self, d, H, W, flags=0, rows=(0, 0), mats_transposed=0, seed=0):
        """-> R (what the call returns), color, depth ([B,2,H,W] with DMR_FLAG_ALPHA), fragments (the body of
        DMR_BUF_TRI_FRAGMENTS, uint8, or None), log, args"""
        sc, a, keep = self.scene(d, H, W, flags, rows, mats_transposed, seed)
        self._begin()
        color, pc = self.output((sc.B, 3, H, W), "out_color")
        depth, pd = self.output((sc.B, 2 if flags & self.capi.FLAG_ALPHA else 1, H, W), "out_depth")
        R = C.c_int(0)
        rc = self.lib.dmr_tri_forward(C.byref(sc), pc, pd, self.alloc_fn, None, None, C.byref(R))
        self._end(rc, True)
        return _Result(R=R.value, color=color, depth=depth, fragments=self.served.get(self.capi.BUF_TRI_FRAGMENTS), log=list(self.log), args=a)

    def tri_backward(self, d, H, W, flags, R, gc, gd, rows=(0, 0), mats_transposed=0, seed=0):
        """The backward of the last forward (same scene) -> grads [dL_dverts, dL_dvcolor, dL_dfopacity, dL_dvdepth, dL_dfintense],
        camera (the body of DMR_BUF_TRI_CAMERA_GRADS or None), log"""
        sc, a, keep = self.scene(d, H, W, flags, rows, mats_transposed, seed)
        gc, gd = self._upstream(gc, gd)
        self._begin()
        B, P, F = sc.B, sc.P, sc.F
        out = [self.output(s, n) for s, n in (((P, 3), "dL_dverts"), ((P, 3), "dL_dvcolor"), ((F,), "dL_dfopacity"),
                                              ((B, P), "dL_dvdepth"), ((B, F), "dL_dfintense"))]
        rc = self.lib.dmr_tri_backward(C.byref(sc), gc.data_ptr(), gd.data_ptr(), int(R), *self._scratch_ptrs(), *[p for _, p in out],
                                       self.alloc_fn, None, None)
        self._end(rc, False)
        return _Result(grads=[t for t, _ in out], camera=self.served.get(self.capi.BUF_TRI_CAMERA_GRADS), log=list(self.log))

    def tet_forward(self, d, H, W, flags=0, rows=(0, 0), mats_transposed=0, seed=0):
        """-> R, color, depth, active, fragments (the body of DMR_BUF_TET_FRAGMENTS or None), log, args"""
        sc, a, keep = self.scene(d, H, W, flags, rows, mats_transposed, seed, tet=True)
        self._begin()
        color, pc = self.output((sc.B, 3, H, W), "out_color")
        depth, pd = self.output((sc.B, 2 if flags & self.capi.FLAG_ALPHA else 1, H, W), "out_depth")
        active, pa = self.output((sc.B, H, W), "out_active")
        R = C.c_int(0)
        rc = self.lib.dmr_tet_forward(C.byref(sc), pc, pd, pa, self.alloc_fn, None, None, C.byref(R))
        self._end(rc, True)
        return _Result(R=R.value, color=color, depth=depth, active=active, fragments=self.served.get(self.capi.BUF_TET_FRAGMENTS),
                       log=list(self.log), args=a)

    def tet_backward(self, d, H, W, flags, gc, gd, rows=(0, 0), mats_transposed=0, seed=0):
        """The backward of the last forward (same scene) -> grads [dL_dvcolor, dL_dfopacity], full (the body of DMR_BUF_TET_GRADS
        or None), camera (the body of DMR_BUF_TET_CAMERA_GRADS or None), log"""
        sc, a, keep = self.scene(d, H, W, flags, rows, mats_transposed, seed, tet=True)
        gc, gd = self._upstream(gc, gd)
        self._begin()
        out = [self.output((sc.P, 3), "dL_dvcolor"), self.output((sc.F,), "dL_dfopacity")]
        rc = self.lib.dmr_tet_backward(C.byref(sc), gc.data_ptr(), gd.data_ptr(), *self._scratch_ptrs(), *[p for _, p in out],
                                       self.alloc_fn, None, None)
        self._end(rc, False)
        return _Result(grads=[t for t, _ in out], full=self.served.get(self.capi.BUF_TET_GRADS),
                       camera=self.served.get(self.capi.BUF_TET_CAMERA_GRADS), log=list(self.log))


class GuardedTriCalls(GuardedCalls):
    """The default tri calls of GuardedCalls under their earlier names (body fill 0xA5, outputs pre-filled with NaN)."""

    def forward(self, d, B, H, W, flags):
        """-> (the R the call returns, colour, depth, the call's tensor arguments); flags: DMR_FLAG_ASYNC = 1"""
        r = self.tri_forward(d, H, W, flags)
        assert r.color.shape[0] == B
        return r.R, r.color, r.depth, r.args

    def backward(self, d, B, H, W, flags, R, gc, gd):
        """The backward of the last forward (same scene): -> [dL_dverts, dL_dvcolor, dL_dfopacity, dL_dvdepth, dL_dfintense]"""
        return self.tri_backward(d, H, W, flags, R, gc, gd).grads
