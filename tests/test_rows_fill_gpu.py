"""The row units' fill kernel (csrc/dmr_rows_common.hip: k_rows_fill behind rows_fill_on) through the C ABI, into a slice of a
larger buffer that holds a non-zero pattern: every word of the slice gets the value, the words in front of and behind it keep
the pattern.  The launch is capped at 4096 workgroups of 256, so more than 4096 * 256 words take a second grid-stride trip,
which no case table of the units reaches; the sizes here lie around a workgroup, around the cap and past twice the cap.
  dmr_packed_row_views fills view_out with -1 before its walk writes the owned rows: one slot (B = K = H = W = 1) that owns no
    row leaves all N words -1, the same slot owning row N - 1 leaves the last word 0.
  dmr_hashgrid_rows_backward with N = 0 and dL_dtable alone launches nothing but the fill with 0.
"""
import ctypes as C

import pytest
import torch as th

import capi_ctypes
from row_units import declare

pytestmark = pytest.mark.gpu

CAP = 4096 * 256          # the words one trip of the capped grid stores
PATTERN = 0x5A5A5A5A      # (as float32 3.8e16: neither 0 nor -1)
FRONT, BACK = 7, 300      # words around the slice (its first word is off a 16-byte boundary)
SIZES = [1, 255, 256, 257, CAP, CAP + 1, 2 * CAP + 54]


def _library():
    return declare(capi_ctypes.load(), ["dmr_packed_row_views", "dmr_hashgrid_layout", "dmr_hashgrid_rows_backward"])


def _buffer(n):
    """int32 [FRONT + n + BACK] on the GPU holding PATTERN, and the address of its slice's first word"""
    buf = th.full((FRONT + n + BACK,), PATTERN, dtype=th.int32, device="cuda")
    return buf, buf.data_ptr() + 4 * FRONT


def _around_kept(buf, n):
    return bool((buf[:FRONT] == PATTERN).all() and (buf[FRONT + n:] == PATTERN).all())


@pytest.mark.parametrize("N", SIZES)
def test_row_views_fill_every_word_of_the_slice(N):
    lib = _library()
    for owned in (-1, N - 1):
        row = th.tensor([owned], dtype=th.int32, device="cuda").reshape(1, 1, 1, 1)
        buf, out = _buffer(N)
        th.cuda.synchronize()
        assert lib.dmr_packed_row_views(1, 1, 1, 1, N, row.data_ptr(), out, None) == 0, capi_ctypes.last_error()
        th.cuda.synchronize()
        got = buf[FRONT:FRONT + N]
        filled = N if owned < 0 else N - 1
        assert int((got[:filled] == -1).sum()) == filled and _around_kept(buf, N), (N, owned)
        assert owned < 0 or int(got[-1]) == 0


def test_hashgrid_backward_without_rows_zeroes_the_whole_table():
    lib = _library()
    L, F, log2_T = 2, 2, 20
    res = (C.c_int32 * L)(2, 65536)
    offsets = (C.c_int64 * (L + 1))()
    assert lib.dmr_hashgrid_layout(L, log2_T, res, offsets) == 0, capi_ctypes.last_error()
    floats = offsets[L] * F
    assert floats > CAP and floats % 256 != 0 and offsets[L] == 27 + (1 << 20)   # (a dense 3^3 level and a hashed one)
    buf, out = _buffer(floats)
    th.cuda.synchronize()
    ret = lib.dmr_hashgrid_rows_backward(0, L, F, log2_T, res, None, buf.data_ptr(), None, None, None, out, None)   # (table: non-null, not read)
    assert ret == 0, capi_ctypes.last_error()
    th.cuda.synchronize()
    assert int((buf[FRONT:FRONT + floats] == 0).sum()) == floats and _around_kept(buf, floats)
