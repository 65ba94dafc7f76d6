"""fragments.pack_slots_fused, interpolate_packed_fused and composite_values_packed_fused on the GPU (csrc/dmr_packed.hip: k_pack_count,
k_pack_scan, k_pack_write, k_interpolate_packed, k_interpolate_packed_backward, k_composite_values_packed,
k_composite_values_packed_backward) against fragments.pack_slots (exactly) and against fragments.interpolate_packed /
composite_values_packed evaluated in float64 on the CPU, on the same float32 inputs cast up; against the dense fused unit
(interpolate_fused, composite_values_fused) bit for bit; on rendered lists; and through a replayed HIP graph.

Bounds (the project's own): forward rel_err <= FWD_TOL = 1e-5, gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err); two
evaluations of the same sums in another order <= sum_order_tol(name).  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over all 92 cases (rel_err against the float64 models): interpolate_packed_fused rows
1.8e-7, dL_dvert_attrs 2.7e-7, dL_dbary 2.3e-7; composite_values_packed_fused image 2.4e-7, T 2.0e-7, dL_dfaces_opacity 2.4e-7,
dL_dvalues 1.7e-7, dL_dface_scale 5.0e-7.  pack_slots_fused: row, n_used and rows equal pack_slots' in all 90 (shape, fill,
capacity) combinations.  The misaligned calls give the aligned calls' forwards bit for bit, gradients to 1.1e-7 (bary and values
equal).  Against the dense fused unit: rows, image and T equal bit for bit (no reordering was needed).  Rendered lists: colour to
8.9e-8 (tri, fill 0.27), 6.0e-8 (tet, fill 0.40); verts.grad against the torch path 3.1e-7 (tri, max |ref| 18.5), 1.2e-6 (tet, max
|ref| 42).  Graph replays against eager (used slots 7 254 -> 4 695 -> 9 396 of capacity 9 600): the stored outputs equal, the
accumulated ones to 1.2e-7, exact zeros in the tail rows.
"""
import functools

import numpy as np
import pytest
import torch as th

import packed_cases as PC
import test_deferred_gpu as DG
from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from shading_cases import EDGE_FRAMES, FRAME, NEW_FRAME, SIZES, one_float_in
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
GRADS_I = ("vert_attrs", "bary")                       # interpolate_packed_fused
GRADS_V = ("faces_opacity", "values", "face_scale")    # composite_values_packed_fused


def _used(face, F):
    return (face >= 0) & (face < F)


@functools.lru_cache(maxsize=None)
def _case(K, C, size, frame=FRAME, cap=None, extra_f=0):
    """test_deferred_gpu._lists' caller-made lists (15 % of the slots -1, 10 % ids past F, an opacity exactly 1 and one exactly
    0), packed on the CPU for F + extra_f faces with capacity None (cap None) or count + cap, and per-row values and upstreams."""
    d = dict(DG._lists(K, C, size, frame))
    F = d["faces_opacity"].shape[0]
    count = int(_used(d["face"], F + extra_f).sum())
    packed = FG.pack_slots(Fragments(d["face"], None, None), F + extra_f, None if cap is None else count + cap)
    g = th.Generator().manual_seed(17 + K + 100 * C)
    d.update(packed=packed, count=count, pack_f=F + extra_f, capacity=None if cap is None else count + cap,
             values=th.randn(packed.rows, C, generator=g), g_rows=th.randn(packed.rows, C, generator=g))
    return d


def _interp_model(d):
    """fragments.interpolate_packed in float64 on the CPU -> out, {name: grad} (numpy)."""
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS_I}
    out = FG.interpolate_packed(Fragments(d["face"], lv["bary"], None), d["packed"], d["faces"], lv["vert_attrs"])
    (out * th.nan_to_num(d["g_rows"]).double()).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


def _values_model(d, with_scale):
    """fragments.composite_values_packed in float64 on the CPU -> image, T, {name: grad} (numpy)."""
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS_V if with_scale or k != "face_scale"}
    image, T = FG.composite_values_packed(Fragments(d["face"], None, None), d["packed"], lv["faces_opacity"], lv["values"], lv.get("face_scale"))
    ((image * d["g_image"].double()).sum() + (T * d["g_T"].double()).sum()).backward()
    return image.detach().numpy(), T.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _interp_reference(*key):
    return _interp_model(_case(*key))


@functools.lru_cache(maxsize=None)
def _values_reference(with_scale, *key):
    return _values_model(_case(*key), with_scale)


def _pack_on(d, dev):
    """pack_slots_fused on the device: row, n_used and rows are the CPU model's, exactly."""
    p = FG.pack_slots_fused(Fragments(d["face"].to(dev), None, None), d["pack_f"], d["capacity"])
    assert p.rows == d["packed"].rows and th.equal(p.row.cpu(), d["packed"].row) and th.equal(p.n_used.cpu(), d["packed"].n_used)
    return p


def _interp_fused(d, dev, want=GRADS_I, leaves=None):
    """interpolate_packed_fused on the device, gradients of `want` only -> out, {name: grad}."""
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "vert_attrs", "g_rows")}
    lv = {k: (leaves[k].detach() if leaves and k in leaves else t[k].clone()).requires_grad_(True) for k in want}
    out = FG.interpolate_packed_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), _pack_on(d, dev), t["faces"],
                                      lv.get("vert_attrs", t["vert_attrs"]))
    grads = th.autograd.grad(out, [lv[k] for k in want], grad_outputs=t["g_rows"]) if want else ()
    return out.detach(), dict(zip(want, grads))


def _values_fused(d, dev, with_scale, want=GRADS_V, leaves=None):
    """composite_values_packed_fused on the device, gradients of `want` only -> image, T, {name: grad}."""
    t = {k: d[k].to(dev) for k in ("face", "faces_opacity", "values", "face_scale", "g_image", "g_T")}
    names = [k for k in want if with_scale or k != "face_scale"]
    lv = {k: (leaves[k].detach() if leaves and k in leaves else t[k].clone()).requires_grad_(True) for k in names}
    image, T = FG.composite_values_packed_fused(Fragments(t["face"], None, None), _pack_on(d, dev), lv.get("faces_opacity", t["faces_opacity"]),
                                                lv.get("values", t["values"]), lv.get("face_scale", t["face_scale"]) if with_scale else None)
    grads = th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [lv[k] for k in names]) if names else ()
    return image.detach(), T.detach(), dict(zip(names, grads))


def _counting(d):
    """[B,K,H,W] bool: the slots that count in a call with the lists' own F."""
    row = d["packed"].row
    return (row >= 0) & (row < d["packed"].rows) & _used(d["face"], d["faces_opacity"].shape[0])


def _free_rows(d):
    """[N] bool: the rows no counting slot holds (the tail, and the rows of slots that are empty for the call)."""
    free = th.ones(d["packed"].rows, dtype=th.bool)
    free[d["packed"].row[_counting(d)].long()] = False
    return free


def _check_interp(tag, d, ref, got):
    out_r, g_r = ref
    out, g = got
    for k, r in dict(g_r, out=out_r).items():
        assert float(np.abs(r).max()) > 0, k
    assert tuple(out.shape) == out_r.shape == (d["packed"].rows, d["vert_attrs"].shape[1]) and out.dtype == th.float32
    e = rel_err(out.cpu().numpy(), out_r)
    print(f"\n{tag}: interpolate_packed out {e:.2e} (max |out| {np.abs(out_r).max():.3g}, {d['count']} used slots, {out.shape[0]} rows)")
    assert e <= FWD_TOL
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32
        eg = rel_err(x, r)
        print(f"  dL_d{k} {eg:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert eg <= GRAD_TOL, (k, eg)
    free, dead = _free_rows(d), ~_counting(d)
    if bool(free.any()):  # exact zeros in the tail rows and in the rows of slots that do not count
        assert float(out.cpu()[free].abs().max()) == 0.0
    if bool(dead.any()):  # ... and in dL/dbary of empty and dropped slots
        assert float(g["bary"].cpu()[dead[:, :, None].expand(-1, -1, 2, -1, -1)].abs().max()) == 0.0


def _check_values(tag, d, ref, got):
    image_r, T_r, g_r = ref
    image, T, g = got
    for k, r in dict(g_r, image=image_r, T=T_r).items():
        assert float(np.abs(r).max()) > 0, k
    assert tuple(image.shape) == image_r.shape and tuple(T.shape) == T_r.shape and image.dtype == T.dtype == th.float32
    ei, eT = rel_err(image.cpu().numpy(), image_r), rel_err(T.cpu().numpy(), T_r)
    print(f"\n{tag}: composite_values_packed image {ei:.2e} T {eT:.2e} (max |image| {np.abs(image_r).max():.3g})")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32
        eg = rel_err(x, r)
        print(f"  dL_d{k} {eg:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert eg <= GRAD_TOL, (k, eg)
    free = _free_rows(d)
    if bool(free.any()):  # exact zeros in dL/dvalues
        assert float(g["values"].cpu()[free].abs().max()) == 0.0


def _both(tag, dev, key, scales=(True,)):
    d = _case(*key)
    _check_interp(tag, d, _interp_reference(*key), _interp_fused(d, dev))
    for s in scales:
        _check_values(f"{tag} scale {s}", d, _values_reference(s, *key), _values_fused(d, dev, s))


# ---------------------------------------------------------------------------
# (1) pack_slots_fused against pack_slots
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", PC.PACK_FILLS)
@pytest.mark.parametrize("shape", PC.PACK_SHAPES, ids=["x".join(map(str, s)) for s in PC.PACK_SHAPES])
def test_pack_slots_fused(hip_device, shape, fill):
    """row and n_used equal pack_slots' on the CPU exactly: one slot; one less than, exactly and one more than a workgroup's
    2048; five workgroups; 258 workgroups against the scanner's 256 at a time; capacity None, 0, below, equal to, above the count."""
    F = PC.PACK_F
    g = th.Generator().manual_seed(sum(shape) + len(fill))
    face = th.randint(0, F, shape, generator=g, dtype=th.int32)
    if fill == "mixed":
        r = th.rand(shape, generator=g)
        face = th.where(r < 0.15, th.full_like(face, -1), face)
        face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)
    elif fill == "all_empty":
        face = th.where(face % 2 == 0, th.full_like(face, -1), face + F)
    count = int(_used(face, F).sum())
    assert (count == 0) == (fill == "all_empty") or face.numel() == 1
    frag_c, frag_d = Fragments(face, None, None), Fragments(face.to(hip_device), None, None)
    for capacity in (None, 0, count // 2, count, count + 37):
        want, got = FG.pack_slots(frag_c, F, capacity), FG.pack_slots_fused(frag_d, F, capacity)
        assert got.row.dtype == got.n_used.dtype == th.int32 and got.row.device == got.n_used.device == frag_d.pix_to_face.device
        same = th.equal(got.row.cpu(), want.row) and th.equal(got.n_used.cpu(), want.n_used) and got.rows == want.rows
        print(f"\npack {shape} {fill} capacity {capacity}: {count} used of {face.numel()} slots in {PC.pack_groups(face.numel())} workgroups, "
              f"rows {got.rows}, n_used {int(got.n_used)}, equal {same}")
        assert same and tuple(got.n_used.shape) == (1,) and int(got.n_used) == count


def test_no_rows(hip_device):
    """N == 0 (every slot empty): an empty [0,C] tensor without a launch; the blend gives image 0 and T 1, and zero gradients."""
    dev = hip_device
    d = DG._lists(5, 3, "shared_keys")
    face = th.full_like(d["face"], -1).to(dev)
    frag = Fragments(face, d["bary"].to(dev), None)
    packed = FG.pack_slots_fused(frag, 7)
    assert packed.rows == 0 and int(packed.n_used) == 0 and bool((packed.row == -1).all())
    out = FG.interpolate_packed_fused(frag, packed, d["faces"].to(dev), d["vert_attrs"].to(dev).requires_grad_(True))
    assert tuple(out.shape) == (0, 3) and out.dtype == th.float32 and not out.requires_grad
    o = d["faces_opacity"].to(dev).requires_grad_(True)
    image, T = FG.composite_values_packed_fused(frag, packed, o, out)
    g, = th.autograd.grad(image.sum() + T.sum(), o)
    assert float(image.detach().abs().max()) == 0.0 and bool((T == 1).all()) and float(g.abs().max()) == 0.0
    th.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capacity"):   # capacity=None under stream capture: refused before anything is enqueued
        with th.cuda.graph(th.cuda.CUDAGraph()):
            FG.pack_slots_fused(frag, 7)
    th.cuda.synchronize()


# ---------------------------------------------------------------------------
# (2) the two fused pairs against the float64 models
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("C", PC.LISTS_C)
@pytest.mark.parametrize("K", PC.LISTS_K)
def test_caller_made_lists(hip_device, K, C, size):
    """out, image, T and every gradient against the float64 models: P = 9 (every lane of a wave merges) and P = 9000 (a tile holds
    more vertex rows than the table's 560 slots), partial tiles in both axes, with and without face_scale, opacities exactly 0 and 1."""
    _both(f"K {K} C {C} {size}", hip_device, (K, C, size), (False, True))


@pytest.mark.parametrize("K,C,size", PC.WIDE, ids=[f"K{K}-C{C}-{size}" for K, C, size in PC.WIDE])
def test_wide_rows(hip_device, K, C, size):
    """PACKED_MAX_C with float4 rows and the scalar C below it, on the 17 x 33 view."""
    _both(f"K {K} C {C} {size}", hip_device, (K, C, size, NEW_FRAME))


@pytest.mark.parametrize("K,C,size", PC.MATRIX, ids=[f"K{K}-C{C}-{size}" for K, C, size in PC.MATRIX])
def test_instantiation_matrix(hip_device, K, C, size):
    """Every KMAX of the blend's backward at K == KMAX and at the first K of the next, against float4 rows at CH 4, at CH 8 / 16
    and scalar rows, on the 17 x 33 view.  Where C % 4 == 0, again with vert_attrs and values one float off a 16-byte boundary
    (scalar access) beside the aligned call: forwards bit-equal, gradients within sum_order_tol."""
    dev = hip_device
    key = (K, C, size, NEW_FRAME)
    d = _case(*key)
    own_a, own_v = d["vert_attrs"].to(dev).clone(), d["values"].to(dev).clone()
    assert own_a.data_ptr() % 16 == 0 and own_v.data_ptr() % 16 == 0
    alg_i = _interp_fused(d, dev, leaves={"vert_attrs": own_a})
    alg_v = _values_fused(d, dev, True, leaves={"values": own_v})
    _check_interp(f"K {K} C {C} {size}", d, _interp_reference(*key), alg_i)
    _check_values(f"K {K} C {C} {size}", d, _values_reference(True, *key), alg_v)
    if C % 4 == 0:
        off_a, off_v = one_float_in(own_a), one_float_in(own_v)
        assert off_a.is_contiguous() and off_a.data_ptr() % 16 == 4 and off_v.is_contiguous() and off_v.data_ptr() % 16 == 4
        got_i = _interp_fused(d, dev, leaves={"vert_attrs": off_a})
        got_v = _values_fused(d, dev, True, leaves={"values": off_v})
        _check_interp(f"K {K} C {C} {size} misaligned", d, _interp_reference(*key), got_i)
        _check_values(f"K {K} C {C} {size} misaligned", d, _values_reference(True, *key), got_v)
        same = th.equal(got_i[0], alg_i[0]) and th.equal(got_v[0], alg_v[0]) and th.equal(got_v[1], alg_v[1])
        print(f"misaligned vs aligned: forwards bit-equal: {same}")
        assert same
        for k, a, b in [(k, got_i[1][k], alg_i[1][k]) for k in GRADS_I] + [(k, got_v[2][k], alg_v[2][k]) for k in GRADS_V]:
            e = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print(f"  dL_d{k} misaligned vs aligned {e:.2e}")
            assert e <= sum_order_tol(k), (k, e)


@pytest.mark.parametrize("C", PC.CAPACITY_C)
@pytest.mark.parametrize("cap", (40, -300), ids=("above", "below"))
def test_capacity(hip_device, cap, C):
    """capacity above the count: the tail rows of out and of dL_dvalues are exact zeros, with NaN upstreams and NaN values in
    the tail rows, which nothing may read.  capacity below the count: the dropped slots contribute nothing, and get an exact 0
    in dL_dbary (_check_interp / _check_values assert the zeros; the models drop the same slots)."""
    dev = hip_device
    key = (PC.CAPACITY[0], C, PC.CAPACITY[2], FRAME, cap)
    d = dict(_case(*key))
    N, count = d["packed"].rows, d["count"]
    assert N == count + cap and int((d["packed"].row >= 0).sum()) == min(N, count)
    ref_i, ref_v = _interp_reference(*key), _values_reference(True, *key)
    if cap > 0:
        d["g_rows"], d["values"] = d["g_rows"].clone(), d["values"].clone()
        d["g_rows"][count:], d["values"][count:] = float("nan"), float("nan")
    got_i, got_v = _interp_fused(d, dev), _values_fused(d, dev, True)
    for k, x in list(got_i[1].items()) + list(got_v[2].items()) + [("out", got_i[0]), ("image", got_v[0])]:
        assert bool(th.isfinite(x).all()), k
    _check_interp(f"C {C} capacity {cap:+d}", d, ref_i, got_i)
    _check_values(f"C {C} capacity {cap:+d}", d, ref_v, got_v)
    if cap > 0:
        assert float(got_i[0][count:].abs().max()) == 0.0 and float(got_v[2]["values"][count:].abs().max()) == 0.0
    else:
        dropped = _used(d["face"], 7) & (d["packed"].row < 0)
        assert int(dropped.sum()) == -cap
        assert float(got_i[1]["bary"].cpu()[dropped[:, :, None].expand(-1, -1, 2, -1, -1)].abs().max()) == 0.0


def test_packed_for_a_larger_f(hip_device):
    """A `packed` made with a larger F than the call's: slots with a row whose face id the call does not know.  In bounds, and the
    models' numbers with those slots empty: zero rows of out and of dL_dvalues, an exact 0 in dL_dbary."""
    key = PC.OTHER_F + (FRAME, None, 17)   # (the lists' ids past F end at F + 16)
    d = _case(*key)
    F = d["faces_opacity"].shape[0]
    extra = (d["face"] >= F) & (d["packed"].row >= 0)
    assert int(extra.sum()) > 100 and d["count"] == d["packed"].rows
    _both("packed for F + 17", hip_device, key)


@pytest.mark.parametrize("K,C,size", PC.HAND_MADE, ids=[f"K{K}-C{C}-{size}" for K, C, size in PC.HAND_MADE])
def test_rows_in_another_order(hip_device, K, C, size):
    """A hand-made `packed` whose rows are pack_slots' in REVERSE order (row' = N - 1 - row): the rows of a wave's lanes are no
    contiguous range, so the waves of the staged store shape take the plain stores.  In bounds, and the models' numbers."""
    dev = hip_device
    d = dict(_case(K, C, size))
    p = d["packed"]
    d["packed"] = p._replace(row=th.where(p.row >= 0, p.rows - 1 - p.row, p.row))
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "vert_attrs", "faces_opacity", "face_scale", "values", "g_rows", "g_image", "g_T")}
    packed = FG.PackedSlots(d["packed"].row.to(dev), p.n_used.to(dev), p.rows)
    A, bary = t["vert_attrs"].clone().requires_grad_(True), t["bary"].clone().requires_grad_(True)
    out = FG.interpolate_packed_fused(Fragments(t["face"], bary, None), packed, t["faces"], A)
    got_i = (out.detach(), dict(zip(GRADS_I, th.autograd.grad(out, [A, bary], grad_outputs=t["g_rows"]))))
    lv = {k: t[k].clone().requires_grad_(True) for k in GRADS_V}
    image, T = FG.composite_values_packed_fused(Fragments(t["face"], None, None), packed, lv["faces_opacity"], lv["values"], lv["face_scale"])
    grads = th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [lv[k] for k in GRADS_V])
    _check_interp(f"K {K} C {C} {size}, rows reversed", d, _interp_model(d), got_i)
    _check_values(f"K {K} C {C} {size}, rows reversed", d, _values_model(d, True), (image.detach(), T.detach(), dict(zip(GRADS_V, grads))))


def test_face_with_a_vertex_out_of_range(hip_device):
    """A face whose row of `faces` holds a vertex index outside [0, P): its slots keep their rows, which are exact zeros; an exact
    0 in dL_dbary, nothing scattered into dL_dvert_attrs.  The float64 model receives such a face's slots as -1."""
    K, C, size = PC.BAD_ROWS
    d = dict(_case(K, C, size))
    F, P = SIZES[size]
    faces = d["faces"].clone()
    faces[2, 1], faces[3, 0], faces[5, 2] = P, -1, 2 ** 31 - 1
    hit = _used(d["face"], F) & ((faces < 0) | (faces >= P)).any(1)[d["face"].clamp(0, F - 1).long()]
    assert int(hit.sum()) > 100
    d["faces"] = faces
    dm = dict(d, face=th.where(hit, th.full_like(d["face"], -1), d["face"]), faces=faces.clamp(0, P - 1))
    got = _interp_fused(d, hip_device)
    _check_interp("three faces with a vertex out of range", dm, _interp_model(dm), got)
    assert float(got[0].cpu()[d["packed"].row[hit].long()].abs().max()) == 0.0


@pytest.mark.parametrize("frame", [NEW_FRAME] + EDGE_FRAMES, ids=["x".join(map(str, f)) for f in [NEW_FRAME] + EDGE_FRAMES])
def test_frames(hip_device, frame):
    """The 17 x 33 view, a view of whole tiles only, and views of one pixel."""
    _both(f"frame {frame}", hip_device, (PC.EDGE_K, PC.EDGE_C, "shared_keys", frame))


# ---------------------------------------------------------------------------
# (3) against the dense fused unit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,size", PC.DENSE, ids=[f"K{K}-C{C}-{size}" for K, C, size in PC.DENSE])
def test_against_the_dense_unit(hip_device, K, C, size):
    """interpolate_packed_fused == interpolate_fused(...).permute(0, 1, 3, 4, 2)[row >= 0] and composite_values_packed_fused(v) ==
    composite_values_fused(unpack_values(v)), image and T, BIT FOR BIT: the same expressions in the same order under the same
    contraction."""
    dev = hip_device
    d = _case(K, C, size)
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "vert_attrs", "faces_opacity", "face_scale", "values")}
    frag, packed = Fragments(t["face"], t["bary"], None), _pack_on(d, dev)
    rows = FG.interpolate_packed_fused(frag, packed, t["faces"], t["vert_attrs"])
    dense = FG.interpolate_fused(frag, t["faces"], t["vert_attrs"]).permute(0, 1, 3, 4, 2)[packed.row >= 0]
    print(f"\nK {K} C {C} {size}: packed rows vs the dense unit's, equal {th.equal(rows, dense)} (max |rows| {float(rows.abs().max()):.3g})")
    assert float(dense.abs().max()) > 0 and th.equal(rows, dense)
    for scale in (None, t["face_scale"]):
        image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], t["values"], scale)
        image_d, T_d = FG.composite_values_fused(frag, t["faces_opacity"], FG.unpack_values(frag, packed, t["values"]).contiguous(), scale)
        print(f"  blend, scale {scale is not None}: image equal {th.equal(image, image_d)}, T equal {th.equal(T, T_d)}")
        assert float(image_d.abs().max()) > 0 and th.equal(image, image_d) and th.equal(T, T_d)


# ---------------------------------------------------------------------------
# (4) rendered lists
# ---------------------------------------------------------------------------
def _rendered(dev, r, t, args, name, K):
    """On a renderer's lists (return_fragments=K, fragment_grads=True): the packed chain + T bg is the renderer's colour where
    count <= K (FWD_TOL absolute; pixels whose list holds a face of opacity 1 left out, the tet renderer's one exception), and a
    loss on the packed hit points gives the verts.grad of the same loss through the torch path (fragments.interpolate_packed)."""
    verts = t["verts"].clone().requires_grad_(True)
    out = r(*(verts if k == "verts" else t[k] for k in args))
    color, frag = out[0], out[-1]
    F = t["faces"].shape[0]
    assert frag.bary.requires_grad and tuple(frag.pix_to_face.shape)[1] == K
    packed = FG.pack_slots_fused(frag, F)
    fill = packed.rows / frag.pix_to_face.numel()
    col = FG.interpolate_packed_fused(frag, packed, t["faces"], t["verts_color"])
    comp, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], col, t["faces_intense"])
    mine = comp + T * t["bg"].view(1, 3, 1, 1)
    opaque = ((t["faces_opacity"][frag.pix_to_face.clamp(min=0).long()] == 1) & (frag.pix_to_face >= 0)).any(1)
    keep = ((frag.count <= K) & ~opaque)[:, None]
    assert bool(keep.any()) and packed.rows == int((frag.pix_to_face >= 0).sum()) > 0
    e = float(((mine - color).detach().abs() * keep).max())
    print(f"\n{name}: packed chain + T bg vs the renderer's colour {e:.2e} ({int(keep.sum())} of {keep.numel()} pixels, fill {fill:.3f})")
    assert e <= FWD_TOL
    gp = th.randn(packed.rows, 3, generator=th.Generator().manual_seed(11)).to(dev)
    pos_f = FG.interpolate_packed_fused(frag, packed, t["faces"], verts)
    pos_t = FG.interpolate_packed(frag, packed, t["faces"], verts)
    g_f, = th.autograd.grad((pos_f * gp).sum(), verts, retain_graph=True)
    g_t, = th.autograd.grad((pos_t * gp).sum(), verts)
    ep = rel_err(pos_f.detach().cpu().numpy(), pos_t.detach().cpu().numpy())
    eg = rel_err(g_f.cpu().numpy(), g_t.cpu().numpy())
    print(f"{name}: hit points {ep:.2e}; verts.grad fused vs the torch path {eg:.2e} (max |ref| {float(g_t.abs().max()):.3g})")
    assert float(g_t.abs().max()) > 0 and ep <= FWD_TOL and eg <= GRAD_TOL


def test_rendered_tri_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 80, 112
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TRI_ARGS, "tri", K)


def test_rendered_tet_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 1, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TET_ARGS, "tet", K)


# ---------------------------------------------------------------------------
# (5) graph replay
# ---------------------------------------------------------------------------
CHAIN_GRADS = ("faces_opacity", "vert_attrs", "face_scale", "bary")


def test_graph_replay(hip_device):
    """Forward + backward of pack (capacity=M) -> interpolate -> tanh -> blend captured into one HIP graph and replayed twice
    over lists and inputs rewritten in place, the used count changing between the replays: the stored outputs (rows, image, T,
    dL_drows, dL_dbary, row, n_used) equal the eager ones, the accumulated ones are within sum_order_tol, and the tail rows are
    exact zeros."""
    dev = hip_device
    K, C, size = PC.GRAPH
    d = _case(K, C, size)
    F, P = SIZES[size]
    M = d["face"].numel()   # every slot could be used
    t = {k: d[k].to(dev).clone() for k in ("face", "bary", "faces", "vert_attrs", "faces_opacity", "face_scale", "g_image", "g_T")}
    lv = {k: t[k].clone().requires_grad_(True) for k in CHAIN_GRADS}
    stored, names = ("rows", "image", "T", "dL_drows", "bary"), ("rows", "image", "T", "dL_drows") + CHAIN_GRADS + ("row", "n_used")

    def step():
        frag = Fragments(t["face"], lv["bary"], None)
        packed = FG.pack_slots_fused(frag, F, capacity=M)
        rows = FG.interpolate_packed_fused(frag, packed, t["faces"], lv["vert_attrs"])
        image, T = FG.composite_values_packed_fused(frag, packed, lv["faces_opacity"], th.tanh(rows), lv["face_scale"])
        grads = th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [rows] + [lv[k] for k in CHAIN_GRADS])
        return [rows.detach(), image.detach(), T.detach()] + list(grads) + [packed.row, packed.n_used]

    def same(captured, eager, what):
        by, n = dict(zip(names, captured)), int(captured[-1])
        for k, a, b in zip(names, captured, eager):
            if k in stored or k in ("row", "n_used"):
                eq = th.equal(a, b)
                print(f"\ngraph replay vs eager, {what}, {k}: equal {eq}")
                assert eq, (what, k)
            else:
                e = rel_err(a.cpu().numpy(), b.cpu().numpy())
                print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g})")
                assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (what, k, e)
        assert 0 < n < M and float(by["rows"][n:].abs().max()) == 0.0 and float(by["dL_drows"][n:].abs().max()) == 0.0
        assert float(by["rows"][:n].abs().max()) > 0 and float(by["dL_drows"][:n].abs().max()) > 0
        return n

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.fill_(1)
    replay(graph)
    counts = [same(captured, eager, "the captured inputs")]
    g = th.Generator().manual_seed(5)
    for fraction in (0.5, 0.02):   # half of the slots emptied; then nearly all of them back
        with th.no_grad():
            r = th.rand(d["face"].shape, generator=g)
            t["face"].copy_(th.where(r < fraction, th.full_like(d["face"], -1), th.randint(0, F, d["face"].shape, generator=g, dtype=th.int32)).to(dev))
            lv["bary"].copy_((th.rand(d["bary"].shape, generator=g) * 0.5).to(dev))
            lv["faces_opacity"].copy_((th.rand(F, generator=g) * 0.5 + 0.2).to(dev))
            lv["vert_attrs"].copy_(th.randn(P, C, generator=g).to(dev))
        replay(graph)
        fresh = [x.detach().clone() for x in step()]
        th.cuda.synchronize()
        counts.append(same(captured, fresh, f"lists rewritten in place, {fraction:.0%} emptied"))
    print(f"used slots over the replays: {counts} of capacity {M}")
    assert counts[1] < counts[0] < counts[2] < M


def test_binding_refusals(hip_device):
    """The binding's own refusals, below fragments.py's: every case of shading_cases.binding_refusals("packed") raises a
    RuntimeError with the message the binding gave before its argument builders were put together from shared checks
    (tests/golden/shading_refusals.json: a record of that binding on the GPU over the same cases).  One or two wrong arguments
    per call, at one pixel: no call reaches a kernel."""
    import json
    import os
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")))["binding"]["packed"]
    cases = SC.binding_refusals("packed", hip_device)
    assert sorted({case for case, _, _ in cases}) == sorted(golden)
    for case, call, args in cases:
        with pytest.raises(RuntimeError) as e:
            getattr(_C, call)(*args)
        assert str(e.value) == golden[case], (case, call)
