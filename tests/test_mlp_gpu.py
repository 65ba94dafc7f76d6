"""fragments.mlp_rows_fused and RowMLP on the GPU (csrc/dmr_mlp.hip: k_mlp_rows, k_mlp_rows_backward, k_mlp_reduce) against
fragments.mlp_rows evaluated in float64 on the CPU, on the same float32 inputs cast up: the case table of tests/mlp_cases.py
(every instantiation; N around a wave, a workgroup's tile and the capped grids), x off a 16-byte boundary, a dead relu unit,
n_rows on the device, single gradients, the chain pack -> interpolate -> RowMLP -> blend on rendered lists, and a replayed
HIP graph.

Inputs: x ~ N(0,1), W_l ~ N(0, 1/in_l), b ~ 0.1 N(0,1), upstream ~ N(0,1).  The relu gradient jumps where a hidden
pre-activation crosses 0, so a row whose smallest hidden |z| is below 1e-5 in the float64 model carries no upstream (at most
1 % of a case's rows: asserted).

Bounds (the project's own): forward rel_err <= FWD_TOL = 1e-5, gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err).  Each
case also evaluates mlp_rows in float32 on the CPU and prints its distance from float64 -- the yardstick --, and a case's bound
is the larger of the project's bound and four times that distance; never anything the kernels gave.  Two evaluations of the
same sums in another order: <= sum_order_tol(name).  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over the table's 22 cases (rel_err against the float64 model; in brackets float32
torch on the CPU on the same cases, the yardstick): y 3.1e-7 (3.1e-7), dL_dx 3.1e-7 (3.6e-7), weight gradients 5.0e-7 (1.9e-5),
bias gradients 3.7e-7 (3.2e-6).  The 9 misaligned calls give the aligned calls' outputs bit for bit.  The dead unit's
gradients are exact zeros.  n_rows: with and without it dL_db of the output layer differs by 12.1 and 4.5.  A single gradient
alone: dL_dx and the weights' equal, the biases' to 8.5e-8.  The chains on rendered lists against the torch MLP in the middle
(tri 9 674 rows, of 35 840 with capacity=M; tet 5 472, of 13 824): image 6.0e-8, verts.grad 3.0e-7, the parameters' gradients to
4.1e-6.  Graph replays against eager (n_rows 500 -> 90 -> 700 of 700 rows): y and dL_dx equal, the summed gradients to 1.3e-7,
exact zeros in the tail rows.
"""
import functools

import numpy as np
import pytest
import torch as th

import mlp_cases as MC
from dmesh_renderer_amd import fragments as FG
from dmesh_renderer_amd import scenes
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, check, models, n_rows_counts, within_floors
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

KINK = 1e-5


def _dims(c):
    return [c.Cin] + [c.Hd] * c.nh + [c.Cout]


@functools.lru_cache(maxsize=None)
def _inputs(c, seed=0):
    """float32 CPU tensors of a case: x, weights, biases (None without), upstream -- 0 in the rows at a relu kink."""
    g = th.Generator().manual_seed(1000 * seed + 7 * c.N + 13 * c.Cin + c.Hd + c.nh + c.Cout)
    dims = _dims(c)
    x = th.randn(c.N, c.Cin, generator=g)
    ws = [th.randn(o, i, generator=g) / i ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    bs = [0.1 * th.randn(o, generator=g) if c.bias else None for o in dims[1:]]
    up = th.randn(c.N, c.Cout, generator=g)
    if c.act == "relu" and c.N:
        h, near = x.double(), th.zeros(c.N, dtype=th.bool)
        for w, b in list(zip(ws, bs))[:-1]:
            z = h @ w.double().t() + (0 if b is None else b.double())
            near |= z.abs().min(1).values < KINK
            h = th.relu(z)
        assert int(near.sum()) <= 0.01 * c.N, (c, int(near.sum()))
        up[near] = 0
    return dict(x=x, ws=ws, bs=bs, up=up)


def _names(c):
    return ["x"] + [f"w{l}" for l in range(c.nh + 1)] + ([f"b{l}" for l in range(c.nh + 1)] if c.bias else [])


def _run(f, c, d, device, dtype, n=None, x=None):
    """y and the gradients of x, the weights and the biases as numpy, {name: array}; n: the n_rows count or None."""
    xx = d["x"].to(device, dtype).requires_grad_(True) if x is None else x
    ws = [w.to(device, dtype).requires_grad_(True) for w in d["ws"]]
    bs = [None if b is None else b.to(device, dtype).requires_grad_(True) for b in d["bs"]]
    nr = None if n is None else th.tensor([n], dtype=th.int32, device=device)
    y = f(xx, ws, bs, activation=c.act, out_activation=c.oact, n_rows=nr)
    grads = th.autograd.grad(y, [xx] + ws + [b for b in bs if b is not None], grad_outputs=d["up"].to(device, dtype))
    out = {"y": y.detach().cpu().numpy()}
    out.update({k: v.detach().cpu().numpy() for k, v in zip(_names(c), grads)})
    return out


@functools.lru_cache(maxsize=None)
def _models(c, n=None):
    """fragments.mlp_rows on the CPU in float64 and in float32 -> (reference, {name: (the bound of the case, the yardstick)})."""
    return models(_run, FG.mlp_rows, c, _inputs(c), n, rel_err)


def _check(what, c, got, n=None):
    ref, bounds = _models(c, n)
    assert set(got) == set(ref)
    return check(what, ref, bounds, got, rel_err)


@pytest.mark.parametrize("i", range(len(MC.TABLE)))
def test_table(hip_device, i):
    c = MC.TABLE[i]
    ref = _check(str(c), c, _run(FG.mlp_rows_fused, c, _inputs(c), hip_device, th.float32))
    if c.N:
        assert all(float(np.abs(v).max()) > 0 for v in ref.values())
    else:
        assert ref["y"].shape == (0, c.Cout) and all(float(np.abs(ref[k]).max()) == 0 for k in ref if k not in ("y", "x"))


@pytest.mark.parametrize("i", range(len(MC.MISALIGNED)))
def test_x_one_float_off_a_16_byte_boundary(hip_device, i):
    """The scalar row loads beside the aligned call's float4 loads: the forward bit-equal, the gradients within the bounds."""
    c = MC.MISALIGNED[i]
    d = _inputs(c)
    store = th.zeros(c.N * c.Cin + 1, device=hip_device)
    store[1:] = d["x"].to(hip_device).flatten()
    x = store[1:].view(c.N, c.Cin).requires_grad_(True)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    off = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32, x=x)
    on = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32)
    print(f"\n{c}: y equal {np.array_equal(off['y'], on['y'])}")
    assert np.array_equal(off["y"], on["y"])
    _check(str(c), c, off)


def test_a_dead_relu_unit(hip_device):
    """A hidden unit of all-zero weights and zero bias: its pre-activation is exactly 0, so the derivative must be exactly 0."""
    c = MC.DEAD_UNIT
    d = {k: (list(v) if isinstance(v, list) else v) for k, v in _inputs(c, seed=1).items()}
    k = 5
    d["ws"][0] = d["ws"][0].clone(); d["ws"][0][k] = 0
    d["bs"][0] = d["bs"][0].clone(); d["bs"][0][k] = 0
    got = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32)
    ref = _run(FG.mlp_rows, c, d, "cpu", th.float64)
    within_floors("dead unit", ref, got, rel_err)
    assert float(np.abs(got["w0"][k]).max()) == 0.0 and float(got["b0"][k]) == 0.0 and float(np.abs(got["w1"][:, k]).max()) == 0.0
    assert float(np.abs(ref["w0"][k]).max()) == 0.0 and float(np.abs(got["w0"]).max()) > 0


@pytest.mark.parametrize("which", ("N_ROWS", "N_ROWS_VEC"))
def test_n_rows_on_the_device(hip_device, which):
    """The counts 0, below N, N, above N and negative, NaN in the tail rows of x and of the upstream: exact zeros in the tails of y
    and dL_dx, weight and bias gradients equal to the model's on the first n rows -- and the same case without n_rows differs."""
    c = getattr(MC, which)
    base = _inputs(c)
    for n in n_rows_counts(c.N):
        m = min(max(n, 0), c.N)
        d = dict(base, x=base["x"].clone(), up=base["up"].clone())
        d["x"][m:], d["up"][m:] = float("nan"), float("nan")
        got = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32, n)
        ref = _run(FG.mlp_rows, c, dict(d, x=th.nan_to_num(d["x"]), up=th.nan_to_num(d["up"])), "cpu", th.float64, n)
        within_floors(f"n_rows {n} of {c.N},", ref, got, rel_err)
        assert float(np.abs(got["y"][m:]).sum()) == 0.0 and float(np.abs(got["x"][m:]).sum()) == 0.0
        assert m == 0 or (float(np.abs(got["y"][:m]).max()) > 0 and float(np.abs(got["x"][:m]).max()) > 0)
        if m == 0:
            assert all(float(np.abs(got[k]).max()) == 0.0 for k in got)
    # what capacity=M gives: zeros in the tail rows of x, which the biases turn into outputs -- n_rows must make a difference
    d = dict(base, x=base["x"].clone())
    d["x"][130:] = 0
    a, b = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32, 130), _run(FG.mlp_rows_fused, c, d, hip_device, th.float32)
    last = f"b{c.nh}"
    print(f"\nwith and without n_rows: dL_d{last} differs by {np.abs(a[last] - b[last]).max():.3g}, y tail {np.abs(b['y'][130:]).max():.3g}")
    assert np.abs(a[last] - b[last]).max() > 0.01 and np.abs(b["y"][130:]).max() > 0 and np.abs(a["y"][130:]).max() == 0


def test_only_what_is_asked(hip_device):
    """Each single gradient alone equals the all-gradients call (dL_dx bit for bit, the summed ones within sum_order_tol); an
    output the loss does not use gives None for every input."""
    c = MC.ONLY
    d = _inputs(c)
    everything = _run(FG.mlp_rows_fused, c, d, hip_device, th.float32)
    leaves = [d["x"].to(hip_device)] + [w.to(hip_device) for w in d["ws"]] + [b.to(hip_device) for b in d["bs"]]
    for i, name in enumerate(_names(c)):
        args = [t.clone().requires_grad_(j == i) for j, t in enumerate(leaves)]
        y = FG.mlp_rows_fused(args[0], args[1:c.nh + 2], args[c.nh + 2:], activation=c.act, out_activation=c.oact)
        g, = th.autograd.grad(y, [args[i]], grad_outputs=d["up"].to(hip_device))
        e = rel_err(g.cpu().numpy(), everything[name])
        print(f"\nonly dL_d{name}: {e:.2e} from the all-gradients call")
        assert (np.array_equal(g.cpu().numpy(), everything[name]) if name == "x" else e <= sum_order_tol(name)), name
    args = [t.clone().requires_grad_(True) for t in leaves]
    y = FG.mlp_rows_fused(args[0], args[1:c.nh + 2], args[c.nh + 2:], activation=c.act, out_activation=c.oact)
    assert y.requires_grad
    assert all(g is None for g in th.autograd.grad((args[0] * 2).sum(), args[1:], allow_unused=True))
    assert not FG.mlp_rows_fused(leaves[0], leaves[1:c.nh + 2], leaves[c.nh + 2:], activation=c.act).requires_grad


# ---------------------------------------------------------------------------
# The chain on rendered lists
# ---------------------------------------------------------------------------
def _chain(dev, r, t, args, name, K):
    """pack_slots_fused -> interpolate_packed_fused -> RowMLP -> composite_values_packed_fused on a renderer's lists
    (fragment_grads=True) against the same chain with fragments.mlp_rows in the middle: the image, verts.grad and every MLP
    parameter's gradient, with capacity=None and with capacity=M passing n_rows=packed.n_used."""
    F = t["faces"].shape[0]
    th.manual_seed(4)
    mlp = FG.RowMLP(3, MC.CHAIN["hidden"], 3, n_hidden=MC.CHAIN["n_hidden"], activation=MC.CHAIN["activation"], out_activation="sigmoid").to(dev)
    g_image = None
    for capacity in (None, "M"):
        res = []
        for fused in (True, False):
            verts = t["verts"].clone().requires_grad_(True)
            frag = r(*(verts if k == "verts" else t[k] for k in args))[-1]
            M = None if capacity is None else frag.pix_to_face.numel()
            packed = FG.pack_slots_fused(frag, F, M)
            n_rows = None if capacity is None else packed.n_used
            x = FG.interpolate_packed_fused(frag, packed, t["faces"], verts)
            if fused:
                rgb = mlp(x, n_rows=n_rows)
            else:
                rgb = FG.mlp_rows(x, list(mlp.weights), list(mlp.biases), activation=mlp.activation, out_activation=mlp.out_activation, n_rows=n_rows)
            image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], rgb)
            if g_image is None:
                g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
            grads = th.autograd.grad((image * g_image).sum(), [verts] + list(mlp.parameters()))
            res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
            used = int(packed.n_used)
        names = ["image", "verts"] + [f"w{l}" for l in range(len(mlp.weights))] + [f"b{l}" for l in range(len(mlp.weights))]
        for k, a, b in zip(names, *res):
            e = rel_err(a, b)
            print(f"\n{name}, capacity {capacity} ({used} rows of {packed.rows}): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
            assert float(np.abs(b).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (name, capacity, k, e)


def test_chain_on_rendered_tri_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 80, 112
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TRI_ARGS, "tri", K)


def test_chain_on_rendered_tet_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 1, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TET_ARGS, "tet", K)


# ---------------------------------------------------------------------------
# Graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """Forward + backward on M rows (what capacity=M gives) with n_rows on the device, captured into one HIP graph and replayed
    over x, weights and n_rows rewritten in place: the stored outputs (y, dL_dx) equal the eager ones, the summed ones (weight
    and bias gradients) are within sum_order_tol, and the tail rows are exact zeros."""
    dev, c = hip_device, MC.GRAPH
    d = _inputs(c)
    x = d["x"].to(dev).requires_grad_(True)
    ws = [w.to(dev).requires_grad_(True) for w in d["ws"]]
    bs = [b.to(dev).requires_grad_(True) for b in d["bs"]]
    up, n_rows = d["up"].to(dev), th.tensor([500], dtype=th.int32, device=dev)
    names = ["y"] + _names(c)

    def step():
        y = FG.mlp_rows_fused(x, ws, bs, activation=c.act, out_activation=c.oact, n_rows=n_rows)
        return [y.detach()] + list(th.autograd.grad(y, [x] + ws + bs, grad_outputs=up))

    def same(captured, eager, what):
        n = int(n_rows)
        for k, a, b in zip(names, captured, eager):
            if k in ("y", "x"):
                print(f"\ngraph replay vs eager, {what}, {k}: equal {th.equal(a, b)}")
                assert th.equal(a, b), (what, k)
                assert float(a[n:].abs().sum()) == 0.0 and float(a[:n].abs().max()) > 0
            else:
                e = rel_err(a.cpu().numpy(), b.cpu().numpy())
                print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g})")
                assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (what, k, e)

    graph, captured, eager = capture_replay(step)
    for t in captured:
        t.fill_(1)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(9)
    for n in (90, c.N):
        with th.no_grad():
            x.copy_(th.randn(c.N, c.Cin, generator=g).to(dev))
            for w in ws:
                w.copy_((th.randn(w.shape, generator=g) / w.shape[1] ** 0.5).to(dev))
            n_rows.fill_(n)
        replay(graph)
        fresh = [t.detach().clone() for t in step()]
        th.cuda.synchronize()
        same(captured, fresh, f"x, weights and n_rows = {n} rewritten in place")
