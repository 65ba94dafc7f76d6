"""fragments.mlp_rows / mlp_rows_fused / RowMLP without a GPU: the torch model is nn.Sequential's numbers to 1e-12 in float64
(outputs and every gradient), its n_rows rule is what the docstring says (the MLP of x[:n] padded with zeros; a NaN in the tail
rows reaches nothing), RowMLP round-trips through nn.Sequential, the library exports what include/dmesh_renderer_amd_mlp.h
declares and the build lists hold the new files, the functional layer and the C ABI refuse what the kernels do not take --
before anything reaches a device, in their documented order -- and the case table of the GPU tests (tests/mlp_cases.py)
reaches every kernel instantiation the unit compiles."""
import itertools

import pytest
import torch as th

import mlp_cases as MC
import row_units as RU
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from row_units import D

UNIT_TEXT, HEADER_TEXT = RU.unit_texts("dmr_mlp.hip", "dmesh_renderer_amd_mlp.h")
FUNCTIONS = ["dmr_mlp_rows", "dmr_mlp_rows_backward"]
TORCH_PATH = r"fragments\.mlp_rows is the torch path"


# ---------------------------------------------------------------------------
# The torch model
# ---------------------------------------------------------------------------
def _sequential(c_in, hidden, c_out, nh, act, oact, bias, seed=0):
    th.manual_seed(seed)
    dims = [c_in] + [hidden] * nh + [c_out]
    mods = []
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        mods.append(th.nn.Linear(i, o, bias=bias))
        if l < nh:
            mods.append(th.nn.ReLU() if act == "relu" else th.nn.Tanh())
    if oact == "sigmoid":
        mods.append(th.nn.Sigmoid())
    return th.nn.Sequential(*mods).double()


def _params(seq):
    lin = [m for m in seq if isinstance(m, th.nn.Linear)]
    return [l.weight for l in lin], [l.bias for l in lin]


@pytest.mark.parametrize("act,oact,nh,bias", list(itertools.product(("relu", "tanh"), ("none", "sigmoid"), (1, 2), (True, False))))
def test_model_against_sequential(act, oact, nh, bias):
    """mlp_rows == the same nn.Sequential in float64 to 1e-12: the output and the gradients of x, every weight and every bias."""
    seq = _sequential(5, 7, 3, nh, act, oact, bias)
    g = th.Generator().manual_seed(1)
    x0, up = th.randn(11, 5, generator=g, dtype=th.float64), th.randn(11, 3, generator=g, dtype=th.float64)
    weights, biases = _params(seq)
    res = []
    for f in (lambda x: seq(x), lambda x: FG.mlp_rows(x, weights, biases, activation=act, out_activation=oact)):
        x = x0.clone().requires_grad_(True)
        y = f(x)
        res.append([y.detach()] + list(th.autograd.grad((y * up).sum(), [x] + list(seq.parameters()))))
    assert len(res[0]) == 2 + (nh + 1) * (2 if bias else 1)
    for a, b in zip(*res):
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-12


def test_model_in_other_dtypes_and_with_mixed_biases():
    seq = _sequential(4, 6, 2, 2, "tanh", "none", True)
    weights, biases = _params(seq)
    x = th.randn(5, 4, dtype=th.float64)
    y = FG.mlp_rows(x.float(), [w.float() for w in weights], [biases[0].float(), None, biases[2].float()], activation="tanh")
    seq[2].bias.data.zero_()
    assert y.dtype == th.float32 and float((y.double() - seq(x)).detach().abs().max()) <= 1e-5


@pytest.mark.parametrize("n", (0, 4, 11, 15, -3))
def test_n_rows_of_the_model(n):
    """The MLP of x[:n] padded with zeros; NaN in the tail rows of x and of the upstream reaches no output and no gradient;
    n_rows above N is N, a negative one 0."""
    seq = _sequential(5, 7, 3, 2, "tanh", "sigmoid", True)
    weights, biases = _params(seq)
    g = th.Generator().manual_seed(2)
    N, m = 11, min(max(n, 0), 11)
    x0, up = th.randn(N, 5, generator=g, dtype=th.float64), th.randn(N, 3, generator=g, dtype=th.float64)
    x0[m:], up[m:] = float("nan"), float("nan")
    x = x0.clone().requires_grad_(True)
    y = FG.mlp_rows(x, weights, biases, activation="tanh", out_activation="sigmoid", n_rows=th.tensor([n], dtype=th.int32))
    assert tuple(y.shape) == (N, 3) and bool(th.isfinite(y).all()) and float(y[m:].detach().abs().sum()) == 0.0
    grads = th.autograd.grad(y, [x] + list(seq.parameters()), grad_outputs=up)   # (the upstream's tail rows are NaN)
    xr = x0[:m].clone().requires_grad_(True)
    yr = seq(xr)
    ref = th.autograd.grad((yr * up[:m]).sum(), [xr] + list(seq.parameters())) if m else None
    assert float((y[:m] - yr).detach().abs().max() if m else 0.0) <= 1e-12
    for k, a in enumerate(grads):
        assert bool(th.isfinite(a).all()), k
        if k == 0:
            assert float(a[m:].abs().sum()) == 0.0
            a = a[:m]
        d = a - ref[k] if m else a
        assert (float(d.abs().max()) if d.numel() else 0.0) <= 1e-12, k


def test_row_mlp_round_trips():
    for nh, act, oact, bias in ((1, "relu", "none", True), (2, "tanh", "sigmoid", False), (2, "relu", "sigmoid", True)):
        seq = _sequential(6, 16, 3, nh, act, oact, bias, seed=3)
        m = FG.RowMLP.from_sequential(seq)
        assert (m.activation, m.out_activation, len(m.weights), m.biases is not None) == (act, oact, nh + 1, bias)
        assert all(a is b for a, b in zip(m.parameters(), _params(seq)[0] + ([b for b in _params(seq)[1]] if bias else [])))  # shared
        x = th.randn(9, 6, dtype=th.float64)
        assert th.equal(m(x), seq(x)) and th.equal(m.to_sequential()(x), seq(x))
        assert [type(a) for a in m.to_sequential()] == [type(a) for a in seq]
        n = th.tensor([4], dtype=th.int32)
        assert th.equal(m(x, n_rows=n), FG.mlp_rows(x, *_params(seq), activation=act, out_activation=oact, n_rows=n))
    fresh = FG.RowMLP(5, 32, 3, n_hidden=2, activation="tanh", bias=True)
    assert [tuple(w.shape) for w in fresh.weights] == [(32, 5), (32, 32), (3, 32)] and [tuple(b.shape) for b in fresh.biases] == [(32,), (32,), (3,)]
    assert len(list(fresh.parameters())) == 6 and len(list(FG.RowMLP(5, 16, 3, bias=False).parameters())) == 2
    bound = 1 / 5 ** 0.5   # nn.Linear's initialisation: U(-1/sqrt(in), 1/sqrt(in))
    assert float(fresh.weights[0].detach().abs().max()) <= bound and float(fresh.biases[0].detach().abs().max()) <= bound
    for bad in (th.nn.Sequential(th.nn.Linear(3, 4)), th.nn.Sequential(th.nn.Linear(3, 4), th.nn.GELU(), th.nn.Linear(4, 2)),
                th.nn.Sequential(th.nn.Linear(3, 4), th.nn.ReLU(), th.nn.Linear(4, 4), th.nn.Tanh(), th.nn.Linear(4, 2)),
                th.nn.Sequential(th.nn.Linear(3, 4), th.nn.ReLU(), th.nn.Linear(4, 8), th.nn.ReLU(), th.nn.Linear(8, 2))):
        with pytest.raises(ValueError, match="RowMLP.from_sequential"):
            FG.RowMLP.from_sequential(bad)
    with pytest.raises(ValueError, match="n_hidden must be 1 or 2"):
        FG.RowMLP(3, 16, 3, n_hidden=3)


# ---------------------------------------------------------------------------
# Library and build lists
# ---------------------------------------------------------------------------
def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, FUNCTIONS)


def test_the_source_and_header_are_build_dependencies():
    RU.are_build_dependencies("dmr_mlp.hip", "dmesh_renderer_amd_mlp.h")


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_MLP is True
    assert callable(_C.mlp_rows) and callable(_C.mlp_rows_backward)
    for n in ("mlp_rows", "mlp_rows_fused", "RowMLP"):
        assert n in FG.__all__ and callable(getattr(FG, n))
    assert FG._FUSED["mlp_rows"][0] == "SUPPORTS_FRAGMENT_MLP"
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(N=6, c_in=3, hidden=16, c_out=3, nh=1, dtype=th.float32):
    dims = [c_in] + [hidden] * nh + [c_out]
    return th.zeros(N, c_in, dtype=dtype), [th.zeros(o, i, dtype=dtype) for i, o in zip(dims[:-1], dims[1:])], [th.zeros(o, dtype=dtype) for o in dims[1:]]


def test_an_older_binding_says_rebuild(monkeypatch):
    class Old:
        SUPPORTS_FRAGMENT_PACKED = True

    x, w, b = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"mlp_rows_fused.*no fused row MLP: rebuild.*" + TORCH_PATH):
        FG.mlp_rows_fused(x, w, b)
    with pytest.raises(TypeError, match="rebuild"):   # ... before any other check
        FG.mlp_rows_fused(x, w[:1], b)
    Old.SUPPORTS_FRAGMENT_MLP = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.mlp_rows_fused(x, w, b)


def test_refusals_in_their_documented_order():
    """The arguments (ValueError, both paths), the fused limits (ValueError naming mlp_rows), dtypes, then devices (TypeError)."""
    x, w, b = _inputs(nh=2)
    for f, name in ((FG.mlp_rows, "mlp_rows"), (FG.mlp_rows_fused, "mlp_rows_fused")):
        with pytest.raises(ValueError, match=rf"{name}: weights must hold 2 or 3 tensors"):
            f(x, w[:1], b[:1])
        with pytest.raises(ValueError, match=rf"{name}: weights must hold 2 or 3 tensors"):
            f(x, w + w[1:2], b + b[1:2])
        with pytest.raises(ValueError, match=rf"{name}: biases must hold one entry"):
            f(x, w, b[:2])
        with pytest.raises(ValueError, match=rf"{name}: activation must be one of"):
            f(x, w, b, activation="gelu")
        with pytest.raises(ValueError, match=rf"{name}: out_activation must be one of"):
            f(x, w, b, out_activation="tanh")
        with pytest.raises(ValueError, match=rf"{name}: x must be \[N,Cin\]"):
            f(x[0], w, b)
        with pytest.raises(ValueError, match=rf"{name}: weights\[0\] must be \[out,in\] = \(16, 3\)"):
            f(x, [th.zeros(16, 4)] + w[1:], b)
        with pytest.raises(ValueError, match=rf"{name}: weights\[1\] must be \[out,in\] = \(16, 16\)"):
            f(x, [w[0], th.zeros(8, 16), th.zeros(3, 8)], b)
        with pytest.raises(ValueError, match=rf"{name}: biases\[2\] must be \[out\] = \(3,\) or None"):
            f(x, w, b[:2] + [th.zeros(4)])
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, w, b, n_rows=th.zeros(2, dtype=th.int32))
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, w, b, n_rows=3)
        with pytest.raises(ValueError, match=rf"{name}: activation"):   # two at once: the first check wins
            f(x[0], w, b, activation="gelu")
    for hidden in (8, 48, 128):
        xx, ww, bb = _inputs(hidden=hidden)
        with pytest.raises(ValueError, match=rf"mlp_rows_fused: the hidden width must be one of \(16, 32, 64\), got {hidden}.*" + TORCH_PATH):
            FG.mlp_rows_fused(xx, ww, bb)
    for c_in in (0, 65):
        xx, ww, bb = _inputs(c_in=c_in)
        with pytest.raises(ValueError, match=rf"mlp_rows_fused: Cin must be in 1\.\.64, got {c_in}.*" + TORCH_PATH):
            FG.mlp_rows_fused(xx, ww, bb)
    for c_out in (0, 17):
        xx, ww, bb = _inputs(c_out=c_out)
        with pytest.raises(ValueError, match=rf"mlp_rows_fused: Cout must be in 1\.\.16, got {c_out}.*" + TORCH_PATH):
            FG.mlp_rows_fused(xx, ww, bb)
    xx, ww, bb = _inputs(hidden=48, dtype=th.float64)   # a bad width and a bad dtype: the width is refused first
    with pytest.raises(ValueError, match="hidden width"):
        FG.mlp_rows_fused(xx, ww, bb)
    with pytest.raises(TypeError, match=r"mlp_rows_fused: x must be float32, got torch.float64; " + TORCH_PATH):
        FG.mlp_rows_fused(x.double(), w, b)
    with pytest.raises(TypeError, match=r"mlp_rows_fused: weights\[1\] must be float32.*" + TORCH_PATH):
        FG.mlp_rows_fused(x, [w[0], w[1].half(), w[2]], b)
    with pytest.raises(TypeError, match=r"mlp_rows_fused: biases\[0\] must be float32.*" + TORCH_PATH):
        FG.mlp_rows_fused(x, w, [b[0].double(), None, None])
    with pytest.raises(TypeError, match=r"mlp_rows_fused: n_rows must be int32, got torch.int64; " + TORCH_PATH):
        FG.mlp_rows_fused(x, w, b, n_rows=th.zeros(1, dtype=th.int64))
    with pytest.raises(TypeError, match=r"mlp_rows_fused: x is on cpu: every tensor must be on one HIP device.*" + TORCH_PATH):
        FG.mlp_rows_fused(x, w, b, n_rows=th.zeros(1, dtype=th.int32))
    for call in (lambda: dmr._C.mlp_rows(x, w, b, 0, 0, None), lambda: dmr._C.mlp_rows_backward(x, w, b, 0, 0, None, x, True, [True] * 3, [True] * 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):   # the binding below it refuses them too
            call()
    m = FG.RowMLP(3, 48, 3)
    assert tuple(m(x).shape) == (6, 3)   # a CPU tensor takes the torch path, whatever the width


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with pointers that are never dereferenced (as tests/test_packed_cpu.py): every check
# runs before any HIP call.  No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
INTS = "N Cin Hd Cout n_hidden act oact"
PTRS = {"dmr_mlp_rows": "x W_in b_in W_mid b_mid W_out b_out n_rows y",   # (scratch_floats: the int64 between scratch and the stream, 0 unless a case sets it)
        "dmr_mlp_rows_backward": "x W_in b_in W_mid b_mid W_out b_out n_rows grad_out dL_dx dL_dW_in dL_db_in dL_dW_mid dL_db_mid dL_dW_out dL_db_out scratch scratch_floats"}
SIZES = dict(N=1, Cin=3, Hd=16, Cout=3, n_hidden=2, act=0, oact=0)
NULL_BY_DEFAULT = ("n_rows", "dL_dx", "dL_dW_in", "dL_db_in", "dL_dW_mid", "dL_db_mid", "dL_dW_out", "dL_db_out", "scratch")
EVERY_CALL = {
    "N<0": (dict(N=-1), "bad rows"),
    "Hd=48": (dict(Hd=48), "Hd must be 16, 32 or 64, got 48"), "Hd=0": (dict(Hd=0), "Hd must be 16, 32 or 64, got 0"),
    "Cin=0": (dict(Cin=0), "Cin must be in 1..64, got 0"), "Cin=65": (dict(Cin=65), "Cin must be in 1..64, got 65"),
    "Cout=0": (dict(Cout=0), "Cout must be in 1..16, got 0"), "Cout=17": (dict(Cout=17), "Cout must be in 1..16, got 17"),
    "n_hidden=0": (dict(n_hidden=0), "n_hidden must be 1 or 2, got 0"), "n_hidden=3": (dict(n_hidden=3), "n_hidden must be 1 or 2, got 3"),
    "act=2": (dict(act=2), "bad activation"), "oact=-1": (dict(oact=-1), "bad activation"),
    "null x": (dict(x=None), "null x"), "null W_in": (dict(W_in=None), "null weights"), "null W_out": (dict(W_out=None), "null weights"),
    "null W_mid": (dict(W_mid=None), "null weights"),
    # two at once: the first check wins
    "bad rows and bad Hd": (dict(N=-1, Hd=48), "bad rows"), "bad Hd and bad Cin": (dict(Hd=48, Cin=0), "Hd must be 16, 32 or 64, got 48"),
    "bad Cin and bad Cout": (dict(Cin=65, Cout=17), "Cin must be in 1..64, got 65"), "bad Cout and null x": (dict(Cout=0, x=None), "Cout must be in 1..16, got 0"),
    "null x and null weights": (dict(x=None, W_in=None), "null x"),
}
PER_CALL = {
    "dmr_mlp_rows": {"null y": (dict(y=None), "null output"), "no rows, null x, null y": (dict(N=0, x=None, y=None), None),
                     "one hidden layer, null W_mid, null y": (dict(n_hidden=1, W_mid=None, y=None), "null output"),
                     "null weights and null y": (dict(W_out=None, y=None), "null weights")},
    "dmr_mlp_rows_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                              "no rows, no gradient wanted": (dict(N=0, x=None, grad_out=None), None),
                              "only dL_dx wanted, no rows": (dict(N=0, x=None, grad_out=None, dL_dx=D), None),
                              "bad Hd although no gradient wanted": (dict(Hd=48), "Hd must be 16, 32 or 64, got 48"),
                              "dL_dW_mid with one hidden layer": (dict(n_hidden=1, dL_dW_mid=D, scratch=D), "a gradient of the second hidden layer without one"),
                              "dL_db_in without b_in": (dict(b_in=None, dL_db_in=D, scratch=D), "the gradient of a bias without the bias"),
                              "null scratch": (dict(dL_dW_in=D), "scratch too small"),
                              "scratch one float short": (dict(dL_db_out=D, scratch=D, scratch_floats=512 * (64 * 16 + 16 + 16 * 16 + 16 + 16 * 16 + 16) - 1), "scratch too small"),
                              "null grad_out and null scratch": (dict(grad_out=None, dL_dW_in=D), "null grad_out")},
}


def test_c_abi_refusals():
    import capi_ctypes
    assert "#define DMR_MLP_TABLE_FLOATS(Hd, n_hidden) (64 * (Hd) + (Hd) + ((n_hidden) == 2 ? (Hd) * (Hd) + (Hd) : 0) + 16 * (Hd) + 16)" in HEADER_TEXT
    RU.run_refusals(RU.declare(capi_ctypes.load(), FUNCTIONS), INTS, PTRS, SIZES, NULL_BY_DEFAULT, EVERY_CALL, PER_CALL, special=dict(scratch_floats=0))


# ---------------------------------------------------------------------------
# The case table of the GPU tests
# ---------------------------------------------------------------------------
def _all_cases():
    return [c for rows in MC.tables().values() for c in rows]


def test_dispatch_restated_as_the_unit_has_it():
    RU.dispatch_restated(MC, UNIT_TEXT, HEADER_TEXT, fills=False)   # (the kernels it launches are the ones every_instantiation lists)
    assert UNIT_TEXT.count("const bool narrow = p.Cout <= 4;") == 2   # (both kernels: the output loops' two widths)
    assert [MC.bwd_threads(hd, nh) for hd in MC.HIDDEN for nh in (1, 2)] == [256, 256, 256, 256, 256, 128]
    assert [MC.vec_of(c, a) for c, a in ((4, True), (4, False), (5, True), (64, True))] == [True, False, False, True]
    assert tuple(FG.MLP_HIDDEN) == MC.HIDDEN


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    assert "k_mlp_reduce<HD, NH><<<" in RU.waits_for_nothing([UNIT_TEXT], fill_calls=0)   # (the partial sums' reduction is a kernel)


def test_table_reaches_every_instantiation():
    full = MC.every_instantiation()
    assert len(full) == 12 + 12 + 6
    reached = MC.instantiations(MC.TABLE)
    assert reached == full, sorted(full - reached, key=str)
    assert MC.instantiations(_all_cases()) == full


def test_table_holds_the_shapes_that_can_go_wrong():
    t = MC.TABLE
    assert {0, 1, 63, 64, 65, 257, 1000} <= {c.N for c in t}
    assert {1, 3, 4, 5, 32, 33, 64} <= {c.Cin for c in t} and {1, 3, 4, 16} <= {c.Cout for c in t}
    assert {c.Hd for c in t} == set(MC.HIDDEN) and {c.nh for c in t} == {1, 2}
    assert {c.act for c in t} == {"relu", "tanh"} and {c.oact for c in t} == {"none", "sigmoid"} and {c.bias for c in t} == {True, False}
    for threads in (128, 256):   # one row more than a backward workgroup's tile
        assert any(c.N == threads + 1 and MC.bwd_threads(c.Hd, c.nh) == threads for c in t)
        assert any(c.N == MC.BWD_MAX_GROUPS * threads + 1 and MC.bwd_threads(c.Hd, c.nh) == threads for c in t)   # ... and one tile more than its grid
    assert any(c.N == MC.FWD_MAX_GROUPS * MC.FWD_THREADS + 1 for c in t)
    assert any(c.Cout <= 4 for c in t) and any(c.Cout > 4 for c in t)   # both widths of the output loops
    assert MC.MISALIGNED and all(c.Cin % 4 == 0 and not c.aligned for c in MC.MISALIGNED) and {c.nh for c in MC.MISALIGNED} == {1, 2}
