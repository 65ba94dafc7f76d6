"""tests/row_units.py without a GPU: each helper the suites of the four row units share fails when it should -- check at and just
above a bound, on a shape and on a NaN; the refusal runner against a stub library written here; the signature table against the
prototypes of the four public headers; waits_for_nothing on texts that wait; the guarded buffers on CPU tensors."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import row_units as RU
from util import rel_err

METRICS = [rel_err, RU.rel_to_largest]
REF = np.array([[0.25, -0.5], [0.125, 0.0625]])   # (max |ref| below 1: the two metrics differ)


@pytest.mark.parametrize("metric", METRICS)
def test_check_at_and_above_the_bound(metric, capsys):
    got = REF + np.array([[0.0, 0.0], [2.0 ** -10, 0.0]])   # (exact in binary)
    e = metric(got, REF)
    assert e == 2.0 ** -10 / (1.0 if metric is rel_err else 0.5)
    assert RU.check("at the bound", {"y": REF}, {"y": (e, 0.0)}, {"y": got}, metric) == {"y": REF}
    assert f"at the bound y: {e:.2e} (float32 torch 0.00e+00, bound {e:.1e}, max |ref| 0.5)" in capsys.readouterr().out
    with pytest.raises(AssertionError):
        RU.check("just above", {"y": REF}, {"y": (np.nextafter(e, 0.0), 0.0)}, {"y": got}, metric)
    with pytest.raises(AssertionError):   # the shape, although every entry is right
        RU.check("shape", {"y": REF}, {"y": (np.inf, 0.0)}, {"y": REF.reshape(1, 2, 2)}, metric)
    with pytest.raises(AssertionError):   # a NaN, whatever the bound
        RU.check("nan", {"y": REF}, {"y": (np.inf, 0.0)}, {"y": np.where(REF == 0.125, np.nan, REF)}, metric)


def test_the_metrics_on_empty_and_all_zero_references():
    empty, zeros = np.zeros((0, 3)), np.zeros(4)
    assert [m(empty, empty) for m in METRICS] == [0.0, 0.0]
    assert RU.rel_to_largest(np.array([0.0, 0.5, 0.0, -0.25]), zeros) == 0.5 and RU.rel_to_largest(zeros, zeros) == 0.0
    big = 8 * REF
    assert RU.rel_to_largest(REF + 0.01, REF) > rel_err(REF + 0.01, REF) and RU.rel_to_largest(big + 0.01, big) == rel_err(big + 0.01, big)


def test_models_bound_is_the_floor_or_four_yardsticks():
    def run(model, case, inputs, device, dtype, n):   # float32 is off by 2^-10 of y and `large`, by 2^-20 of `small`
        assert (model, case, inputs, device, n) == ("model", "case", "inputs", "cpu", 7)
        off = 0.0 if dtype == RU.th.float64 else 2.0 ** -10
        return {"y": REF + off * REF, "small": REF + off * 2.0 ** -10 * REF, "large": REF + off * REF}

    ref, bounds = RU.models(run, "model", "case", "inputs", 7, RU.rel_to_largest)
    assert (RU.FWD_TOL, RU.GRAD_TOL, RU.YARDSTICKS) == (1e-5, 1e-4, 4) and np.array_equal(ref["y"], REF)
    assert bounds == {"y": (2.0 ** -8, 2.0 ** -10), "small": (1e-4, 2.0 ** -20), "large": (2.0 ** -8, 2.0 ** -10)}
    assert RU.models(lambda *a: {"y": REF, "g": REF}, 0, 0, 0, None, rel_err)[1] == {"y": (1e-5, 0.0), "g": (1e-4, 0.0)}


# run_refusals against a library written in Python: two calls that refuse bad rows, a null x, then their own
class Stub:
    error = b""

    def dmr_last_error(self):
        return self.error

    def _answer(self, call, text):
        self.error = b"" if text is None else f"{call}: {text}".encode()
        return 0 if text is None else 1

    def fwd(self, N, x, y, stream):
        assert stream is None and (x is None or x is RU.D)
        return self._answer("fwd", "bad rows" if N < 0 else "null x" if x is None else "null output" if y is None else None)

    def bwd(self, N, x, g, dx, floats, stream):
        assert stream is None and (dx is None or dx is RU.D) and floats in (0, 5)
        return self._answer("bwd", "bad rows" if N < 0 else "null x" if x is None else "null grad_out" if g is None else "too small" if dx and not floats else None)


PTRS = {"fwd": "x y", "bwd": "x g dx floats"}
EVERY_CALL = {"N<0": (dict(N=-1), "bad rows"), "null x": (dict(x=None), "null x"), "bad rows and null x": (dict(N=-2, x=None), "bad rows")}
PER_CALL = {"fwd": {"null y": (dict(y=None), "null output")},
            "bwd": {"null g": (dict(g=None), "null grad_out"), "nothing wanted": (dict(), None), "dx wanted": (dict(dx=RU.D, floats=5), None),
                    "dx without floats": (dict(dx=RU.D), "too small")}}


def _refusals(every_call=EVERY_CALL, per_call=PER_CALL):
    RU.run_refusals(Stub(), "N", PTRS, dict(N=1), ("dx",), every_call, per_call, special=dict(floats=0))


def test_run_refusals_fails_when_it_should():
    _refusals()
    with pytest.raises(AssertionError, match="null x"):       # a text that differs by one character
        _refusals(dict(EVERY_CALL, **{"null x": (dict(x=None), "null X")}))
    with pytest.raises(AssertionError, match="null grad_out"):   # a call that should return 0 returns 1
        _refusals(per_call=dict(PER_CALL, bwd=dict(PER_CALL["bwd"], **{"null g": (dict(g=None), None)})))
    with pytest.raises(AssertionError, match="nothing wanted"):  # ... and one that should refuse returns 0
        _refusals(per_call=dict(PER_CALL, bwd=dict(PER_CALL["bwd"], **{"nothing wanted": (dict(), "null grad_out")})))
    with pytest.raises(AssertionError, match="null y"):       # an argument that one of the calls does not take
        _refusals(dict(EVERY_CALL, **{"null y": (dict(y=None), "null output")}))
    with pytest.raises(AssertionError):                       # cases of a call that is not run: the count is short
        _refusals(per_call=dict(PER_CALL, other={"null y": (dict(y=None), "null output")}))


# The signature table against the public headers
def test_declare_sets_what_the_headers_declare():
    seen = {}
    for unit in ("mlp", "hashgrid", "sh", "envmap"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(RU.ROOT, "include", f"dmesh_renderer_amd_{unit}.h")).read(), flags=re.S)
        mine = {name: [C.c_void_p if "*" in p else C.c_int64 if "int64_t" in p else C.c_int for p in params.split(",")]
                for name, params in re.findall(r"^int (dmr_\w+)\(([^)]*)\);", text, flags=re.M)}
        seen.update(mine)
    assert sorted(seen) == sorted(RU.SIGNATURES) and len(seen) == 10
    lib = SimpleNamespace(dmr_last_error=SimpleNamespace(), **{n: SimpleNamespace() for n in seen})
    assert RU.declare(lib, list(seen)) is lib and lib.dmr_last_error.restype is C.c_char_p
    for name, kinds in seen.items():
        f = getattr(lib, name)
        assert f.restype is C.c_int and f.argtypes == kinds, name
    assert len(lib.dmr_hashgrid_layout.argtypes) == 4 and lib.dmr_mlp_rows_backward.argtypes[-2:] == [C.c_int64, C.c_void_p]
    with pytest.raises(KeyError):
        RU.declare(lib, ["dmr_tri_forward"])   # (not a row unit's call: include/dmesh_renderer_amd.h, tests/capi_ctypes.py)


# The name-parametrised CPU tests
def test_waits_for_nothing_sees_a_wait():
    clean = "void f(hipStream_t st) {\n    rows_fill_on(st, a, n, 0u);  // hipMemset would be a second engine\n    k<<<1, 64, 0, st>>>(a);\n}\n"
    ablation = "#ifdef DMR_ABLATION\nhipMemcpyFromSymbol(out, s, 8);\n#endif\n"
    assert "rows_fill_on(st, a, n, 0u);  \n" in RU.waits_for_nothing([clean, ablation], fill_calls=1)
    for bad in ("hipMemsetAsync(a, 0, n, st);", "hipMemset(a, 0, n);", "while (!*flag) {}", "hipStreamSynchronize(st);", "hipDeviceSynchronize();",
                "hipMalloc(&a, n);", "hipMemcpyAsync(a, b, n, hipMemcpyDeviceToHost, st);", "__builtin_amdgcn_s_sleep(1);", 'asm volatile("");'):
        with pytest.raises(AssertionError):
            RU.waits_for_nothing([clean, bad], fill_calls=1)
    with pytest.raises(AssertionError):   # a second fill, or none
        RU.waits_for_nothing([clean, clean], fill_calls=1)
    with pytest.raises(AssertionError):
        RU.waits_for_nothing([], fill_calls=1)
    RU.waits_for_nothing([clean, "zero_on(st, a, n);"], fill_calls=1)
    with pytest.raises(AssertionError, match="zero_on"):
        RU.waits_for_nothing([clean, "zero_on(st, a, n);"], fill_calls=1, extra_forbidden=["zero_on("])


# GPU patterns, on the CPU
@pytest.mark.parametrize("off", (0, 1, 3))
def test_guarded_and_intact(off):
    n = 10
    buf, body = RU.guarded("cpu", n, off)
    assert (RU.SENTINEL, RU.PAD) == (0x7fc0beef, 64) and len(buf) == 2 * RU.PAD + off + n and tuple(body.shape) == (n,) and body.dtype == RU.th.float32
    assert body.data_ptr() % 16 == (4 * off) % 16 and body.data_ptr() == buf.data_ptr() + 4 * (RU.PAD + off) and bool(body.isnan().all())
    body.fill_(1.0)
    assert RU.intact(buf, n, off) and int((buf == RU.SENTINEL).sum()) == 2 * RU.PAD + off
    for word in (0, RU.PAD + off - 1, RU.PAD + off + n, len(buf) - 1):   # the first and the last word of either side
        buf[word] ^= 1
        assert not RU.intact(buf, n, off), word
        buf[word] ^= 1
    assert RU.intact(buf, n, off) and not RU.intact(buf, n - 1, off) and not RU.intact(buf, n, off + 1)


def test_counts_calls_and_n_rows_counts(monkeypatch):
    binding = SimpleNamespace(rows_backward=lambda a, b=0: a + b)
    calls = RU.counts_calls(monkeypatch, binding, "rows_backward")
    assert calls == [] and binding.rows_backward(2, b=3) == 5 and binding.rows_backward(1) == 1 and calls == [1, 1]
    assert RU.n_rows_counts(300) == (0, 130, 300, 350, -7)
