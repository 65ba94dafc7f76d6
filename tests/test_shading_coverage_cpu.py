"""The fused shading units compile 20 + 10 kernel instantiations, picked at run time from K, C and a pointer's alignment.
Without a GPU: the case tables of their GPU tests (tests/shading_cases.py) together reach every one of them, with float4 and
with scalar loads; the dispatch that claim rests on is still the one in the two .hip files and their common header; and
every new GPU case meets the conditions on its inputs (they depend on the float64 model and the generator alone)."""
import os

import torch as th

import shading_cases as SC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")

# The host code shading_cases restates, line by line.
DISPATCH_LINES = {
    "dmr_shade_common.hpp": [  # what the two units share: the K ladder and the float4 rule, once
        "if (K <= 4) f(std::integral_constant<int, 4>());",
        "else if (K <= 8) f(std::integral_constant<int, 8>());",
        "else if (K <= 16) f(std::integral_constant<int, 16>());",
        "else f(std::integral_constant<int, 32>());",
        "inline int shade_vec(int C, const float* base) { return (C % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0u) ? 1 : 0; }",
    ],
    "dmr_shade.hip": [
        "constexpr int SHADE_MAX_C = 256;",
        "p.vec = shade_vec(C, vert_attrs);",
        "if (C <= 4) k_composite_fragments<4><<<grid, block, 0, st>>>(p, image, T);",
        "else k_composite_fragments<16><<<grid, block, 0, st>>>(p, image, T);",
        "if (p.C <= 4) k_composite_fragments_backward<KMAX, 4><<<",
        "else k_composite_fragments_backward<KMAX, 8><<<",
        "with_kmax(K, [&](auto kmax) {",
        "launch_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dL_dfaces_opacity, dL_dvert_attrs, dL_dface_scale, dL_dbary);",
    ],
    "dmr_texture.hip": [
        "constexpr int TEX_MAX_C = 32;",
        "constexpr int TEX_CHUNKS = TEX_MAX_C / 4;",
        "p.vec = shade_vec(C, texture);",
        "if (C <= 4) k_composite_texture<1><<<grid, block, 0, st>>>(p, image, T);",
        "else k_composite_texture<TEX_CHUNKS><<<grid, block, 0, st>>>(p, image, T);",
        "if (dtex && gi) k_composite_texture_backward<KMAX, true><<<",
        "else k_composite_texture_backward<KMAX, false><<<",
        "with_kmax(K, [&](auto kmax) {",
        "launch_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dL_dfaces_opacity, dL_dvert_uvs, dL_dtexture, dL_dface_scale, dL_dbary);",
    ],
}


def _all_cases():
    return [r for rows in SC.tables().values() for r in rows]


def test_dispatch_restated_as_the_units_have_it():
    """The lines shading_cases mirrors are in the units' files as text, each once: a change of the dispatch fails here until the helper (and
    the tables) follow it.  And the restatement itself, at the thresholds."""
    for name, lines in DISPATCH_LINES.items():
        unit = open(os.path.join(CSRC, name)).read()
        for line in lines:
            assert unit.count(line) == 1, (name, line)
    assert "constexpr int FRAG_MAX_K = 32;" in open(os.path.join(CSRC, "dmr_kernels.hpp")).read()
    assert [SC.kmax_of(K) for K in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]
    assert all(SC.kmax_of(SC.smallest_k(k)) == k and (SC.smallest_k(k) == 1 or SC.kmax_of(SC.smallest_k(k) - 1) < k) for k in SC.KMAXES)
    assert [SC.shade_forward_ch(C) for C in (1, 4, 5, 256)] == [4, 4, 16, 16]
    assert [SC.shade_backward_ch(C) for C in (1, 4, 5, 256)] == [4, 4, 8, 8]
    assert [SC.texture_forward_nch(C) for C in (1, 4, 5, 32)] == [1, 1, 8, 8]
    assert [SC.vec_of(C, a) for C, a in ((4, True), (4, False), (5, True), (8, True), (8, False))] == [1, 0, 0, 1, 0]
    assert SC.tex_of(True) and not SC.tex_of(False) and not SC.tex_of(True, image_upstream=False)


def test_tables_reach_every_instantiation():
    full = SC.every_instantiation()
    assert len(full) == 4 + 16 + 4 + 16
    reached = SC.instantiations(_all_cases())
    assert reached == full, sorted(full - reached)
    # the tables that were there first miss what the later ones are for
    first = SC.instantiations(r for name, rows in SC.tables().items() if name.split(".")[1] in ("caller_made_lists", "only_some", "graph") for r in rows)
    assert len(full - first) == 23 and all(k[1][0] != 16 for k in first if k[0].endswith("backward"))


def test_every_kmax_at_its_ends():
    """Every KMAX of either backward runs at K == KMAX (the last row of tv[KMAX][...]) and at its smallest K."""
    for unit in ("shade", "texture"):
        ks = {r.K for r in _all_cases() if r.unit == unit}
        for kmax in SC.KMAXES:
            assert kmax in ks and SC.smallest_k(kmax) in ks, (unit, kmax)
    # the texture gradient's table (TEX) too, whose size depends on KMAX
    ks = {r.K for r in _all_cases() if r.unit == "texture" and r.tex}
    assert all(kmax in ks and SC.smallest_k(kmax) in ks for kmax in SC.KMAXES)


def test_tables_reach_every_edge():
    for name, reaches in SC.EDGES.items():
        assert any(reaches(r) for r in _all_cases()), name


def test_a_view_one_float_into_a_buffer_is_misaligned():
    """one_float_in on the CPU, whose allocations are 64-byte aligned as the device's are: contiguous, equal, 4 bytes past a
    16-byte boundary.  (The GPU tests assert the same of the device tensor they pass.)"""
    for shape in ((9000, 4), (9000, 8), (7, 13, 32)):
        t = th.randn(*shape)
        v = SC.one_float_in(t)
        assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous() and bool((v == t).all())
        assert v.detach().requires_grad_(True).data_ptr() == v.data_ptr()


def test_new_gpu_cases_meet_their_input_conditions():
    """Every new GPU case: a non-zero float64 reference for every gradient it compares, at most 2 % of the used slots emptied
    near a texel-centre line (texture), opacity and scale gradients above 1 under the merge cases' one-signed upstreams."""
    import test_composite_fused_gpu as S
    import test_composite_texture_gpu as T
    n = 0
    for tag, d, ref, signed in S.new_cases():
        S.check_inputs(d, ref, signed)
        n += 1
    worst = 0.0
    for tag, d, ref, names, signed in T.new_cases():
        T.check_inputs(d, ref, names, signed)
        worst = max(worst, d["removed"])
        n += 1
    print(f"\n{n} cases; at most {100 * worst:.2f} % of the used slots near a texel-centre line")
    assert n == len(SC.SHADE_MATRIX) + len(SC.SHADE_MISALIGNED) + len(SC.TEXTURE_MATRIX) + len(SC.TEXTURE_NO_TEX_GRAD) + len(SC.TEXTURE_MISALIGNED) + 2 + 4
