"""What the suites of the four units over packed rows share (csrc/dmr_mlp.hip, dmr_hashgrid.hip, dmr_sh.hip, dmr_envmap.hip on
csrc/dmr_rows_common.*), each stated once: the error metric, the bound and the comparison of tests/test_*_gpu.py, the ctypes
signatures of the units' C calls, the runner of the C ABI's refusal tables, the four CPU tests that differ only in names, the
guarded buffers, and the lines of the shared source that tests/*_cases.py restate.  Plain functions with arguments, imported
like harness.py and util.py; tests/test_row_units_cpu.py shows that each fails when it should.
"""
import ctypes as C
import os
import re

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmesh_renderer_amd", "csrc")

# The shared source, restated for tests/{mlp,hashgrid,sh,envmap}_cases.py.  COMMON_DISPATCH_LINES: what the units take from
# COMMON_HEADER -- the n_rows clamp, a backward workgroup's run of tiles, the grid, the two ladders behind with_one_of and
# with_wanted and the backward calls' opening --, each there exactly once and in no unit; COMMON_SOURCE defines the fill kernel
# FILL_KERNEL, launched by FILL_LAUNCH_LINE for the units that call rows_fill_on.
COMMON_HEADER, COMMON_SOURCE, FILL_KERNEL = "dmr_rows_common.hpp", "dmr_rows_common.hip", "k_rows_fill"
COMMON_DISPATCH_LINES = [
    "return u < 0 ? 0 : (u > p.N ? p.N : u);",
    '__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");',
    "const int per = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;",
    "return {t0, t0 + per < tiles ? t0 + per : tiles};",
    "const int tiles = (int)(((int64_t)N + threads - 1) / threads);",
    "return {tiles, tiles < max_groups ? tiles : max_groups};",
    "if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>());",
    "else if (v == V) f(std::integral_constant<int, V>());",
    "else with_one_of<Rest...>(v, f);",
    "if (first && second) f(std::true_type(), std::true_type());",
    "else if (first) f(std::true_type(), std::false_type());",
    "else f(std::false_type(), std::true_type());",
    'if (N > 0 && !grad_out) return api_fail((std::string(name) + ": null grad_out").c_str());',
    "if (N == 0) dL_dx = nullptr;  // (no row to write)",
    "return (dL_dx || others) ? SHADE_LAUNCH : SHADE_DONE;",
]
FILL_LAUNCH_LINE = "k_rows_fill<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st>>>(static_cast<uint32_t*>(a), n, value);"
COMMON_TEXT, FILL_TEXT = (open(os.path.join(CSRC, f)).read() for f in (COMMON_HEADER, COMMON_SOURCE))
ABLATION = re.compile(r"#ifdef DMR_ABLATION.*?#endif", re.S)   # (the ablation builds' blocks are not in the product)


def unit_texts(source, header):
    """(the text of csrc/<source>, the text of include/<header>)"""
    return open(os.path.join(CSRC, source)).read(), open(os.path.join(ROOT, "include", header)).read()


# Metrics and bounds.  An output is within max(its floor, YARDSTICKS x the yardstick) of the float64 model on the CPU, the
# yardstick being the float32 model on the CPU against the float64 one on the same case; never anything the kernels gave.
# The metric is the suite's: util.rel_err (error over max(1, max |ref|)) for the MLP and the hash grid, rel_to_largest for the
# SH and envmap units.  rel_to_largest is never the smaller of the two, so they are not interchangeable.
FWD_TOL, GRAD_TOL, YARDSTICKS = 1e-5, 1e-4, 4


def rel_to_largest(got, ref):
    """max |got - ref| / max |ref| (max |got| where the reference is all zeros: such an output must be zeros)."""
    if ref.size == 0:
        return 0.0
    top = float(np.abs(ref).max())
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) / (top if top > 0 else 1.0)


def models(run, model_fn, case, inputs, n, metric, floors=(FWD_TOL, GRAD_TOL)):
    """run(model_fn, case, inputs, "cpu", dtype, n) in float64 and in float32 -> (reference, {name: (the bound, the yardstick)})"""
    ref, f32 = run(model_fn, case, inputs, "cpu", th.float64, n), run(model_fn, case, inputs, "cpu", th.float32, n)
    bounds = {}
    for k in ref:
        yard = metric(f32[k], ref[k])
        bounds[k] = (max(floors[0] if k == "y" else floors[1], YARDSTICKS * yard), yard)
    return ref, bounds


def check(what, reference, bounds, got, metric):
    """Prints what each output of `got` measures and asserts its shape, that it is finite and its bound -> reference."""
    for k in got:
        ref, e, (bound, yard) = reference[k], metric(got[k], reference[k]), bounds[k]
        print(f"\n{what} {k}: {e:.2e} (float32 torch {yard:.2e}, bound {bound:.1e}, max |ref| {float(np.abs(ref).max()) if ref.size else 0:.3g})")
        assert got[k].shape == ref.shape and np.isfinite(got[k]).all() and e <= bound, (what, k, e)
    return reference


def within_floors(what, reference, got, metric):
    """check against the floors alone, for the calls whose model is not a cached case (n_rows, special rows)."""
    for k in reference:
        e = metric(got[k], reference[k])
        print(f"\n{what} {k}: {e:.2e}")
        assert np.isfinite(got[k]).all() and e <= (FWD_TOL if k == "y" else GRAD_TOL), (what, k, e)


# The C calls: name -> (leading ints, pointers with the trailing stream, then whatever else follows them)
SIGNATURES = {
    "dmr_mlp_rows": (7, 10), "dmr_mlp_rows_backward": (7, 17, C.c_int64, C.c_void_p),   # (... scratch, scratch_floats, stream)
    "dmr_hashgrid_layout": (2, 2), "dmr_hashgrid_rows": (4, 6), "dmr_hashgrid_rows_backward": (4, 8),   # (layout: host only, no stream)
    "dmr_packed_row_views": (5, 3), "dmr_sh_rows": (3, 6), "dmr_sh_rows_backward": (3, 8),
    "dmr_envmap_rows": (4, 5), "dmr_envmap_rows_backward": (4, 7),
}


def declare(lib, names):
    """Sets restype and argtypes of `names` (and of dmr_last_error) on a ctypes library, however it was loaded -> lib."""
    for name in names:
        ints, pointers, *rest = SIGNATURES[name]
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [C.c_int] * ints + [C.c_void_p] * pointers + rest
    lib.dmr_last_error.restype = C.c_char_p
    return lib


# The refusal tables of a unit's two calls, through pointers that are never dereferenced
D = C.c_void_p(16)  # non-null, never dereferenced on these paths


def run_refusals(lib, ints, ptrs, sizes, null_by_default, every_call, per_call, special=None):
    """Every case of every_call on each call of ptrs ({call: "the names of what follows the ints"}) and of per_call[call] on its
    own: a case is (changes, text) -- the arguments that differ from the defaults (sizes[name]; special[name], else null where
    null_by_default, else D) and the refusal's text after "<call>: ", or None for a call that returns 0 and enqueues nothing."""
    special, seen = special or {}, set()
    for call, names in ptrs.items():
        takes = ints.split() + names.split()
        for case, (changes, text) in list(every_call.items()) + list(per_call[call].items()):
            assert all(k in takes for k in changes), (call, case)
            args = [changes.get(n, sizes[n]) for n in ints.split()]
            args += [changes.get(n, special.get(n, None if n in null_by_default else D)) for n in names.split()]
            args.append(None)   # stream
            ret = getattr(lib, call)(*args)
            got = lib.dmr_last_error().decode() if ret else ""
            if text is None:
                assert (ret, got) == (0, ""), (call, case, got)
            else:
                assert ret == 1 and got == f"{call}: {text}", (call, case, got)
            seen.add((call, case))
    assert len(seen) == len(ptrs) * len(every_call) + sum(len(v) for v in per_call.values())


# The CPU tests that differ between the units only in names
def exports_declared(header_text, functions, absent=()):
    """The header declares exactly `functions`, the built library exports them, and nothing of `absent`."""
    from dmesh_renderer_amd import build
    assert sorted(set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)))) == functions
    lib = C.CDLL(build.build())
    for n in functions:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    for n in absent:
        assert not hasattr(lib, n), n


def are_build_dependencies(source, header, extra=()):
    """The unit's source, the shared files and the `extra` headers are build dependencies, its public header too; all exist."""
    from dmesh_renderer_amd import build
    assert source in build.SOURCES and COMMON_SOURCE in build.SOURCES and all(h in build.HEADERS for h in (COMMON_HEADER,) + tuple(extra))
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    for deps in (build.HEADERS, build.GLUE_SOURCES, build.PUBLIC_HEADERS):
        assert any(os.path.basename(d) == header for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)
    assert header in build.__doc__


def waits_for_nothing(texts, fill_calls, extra_forbidden=()):
    """The shared source and the unit's `texts`, without comments and ablation blocks: no memset, allocation, copy or wait on the
    host, no spin on a flag, no assembly, and fill_calls calls of rows_fill_on (what a unit zeroes, that kernel fills) -> the code."""
    code = re.sub(r"//[^\n]*", "", ABLATION.sub("", COMMON_TEXT + FILL_TEXT + "".join(texts)))
    for word in ("hipMemset", "hipMalloc", "Synchronize", "hipMemcpy", "while (", "__builtin_amdgcn_s_sleep", "asm") + tuple(extra_forbidden):
        assert word not in code, word
    assert code.count("rows_fill_on(st, ") == fill_calls and FILL_KERNEL + "<<<" in code
    return code


def dispatch_restated(cases, unit_text, header_text, twice=(), fills=True):
    """cases.DISPATCH_LINES are in the unit once (those of `twice`: twice) and not in the shared header, the shared lines the other
    way round, cases.HEADER_LINES in the public header, and the product launches what cases.every_instantiation() lists -> the product."""
    for line in cases.DISPATCH_LINES:
        assert unit_text.count(line) == (2 if line in twice else 1) and COMMON_TEXT.count(line) == 0, line
    for line in twice:
        assert unit_text.count(line) == 2, line
    for line in COMMON_DISPATCH_LINES:
        assert COMMON_TEXT.count(line) == 1 and unit_text.count(line) == 0, line
    assert FILL_TEXT.count(FILL_LAUNCH_LINE) == 1 and '#include "%s"' % COMMON_HEADER in unit_text
    for line in cases.HEADER_LINES:
        assert header_text.count(line) == 1, line
    product = ABLATION.sub("", unit_text)
    launches = lambda text: set(re.findall(r"\b(k_[a-z_]+)(?:<[^<]*>)?<<<", text))
    assert launches(FILL_TEXT) == {FILL_KERNEL} and ("rows_fill_on(st, " in product) == fills
    assert launches(product) | (launches(FILL_TEXT) if fills else set()) == {i[0] for i in cases.every_instantiation()}
    return product


# GPU patterns
SENTINEL, PAD = 0x7fc0beef, 64   # a NaN with a payload; words before and after every body


def guarded(dev, n, off=0):
    """(buffer int32 [PAD + off + n + PAD] of sentinels, its body as float32 [n] starting `off` floats past a 256-byte boundary)"""
    buf = th.full((PAD + off + n + PAD,), SENTINEL, dtype=th.int32, device=dev)
    body = buf[PAD + off:PAD + off + n].view(th.float32)
    assert body.data_ptr() % 16 == (4 * off) % 16
    return buf, body


def intact(buf, n, off=0):
    return bool((buf[:PAD + off] == SENTINEL).all()) and bool((buf[PAD + off + n:] == SENTINEL).all())


def n_rows_counts(N):
    """The n_rows a suite runs on N rows: 0, below N, N, above N and negative; a count n reads m = min(max(n, 0), N) rows."""
    return (0, 130, N, N + 50, -7)


def counts_calls(monkeypatch, _C, name):
    """Wraps the binding's _C.<name> -> the list that grows by a 1 with every call of it."""
    calls, real = [], getattr(_C, name)
    monkeypatch.setattr(_C, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls
