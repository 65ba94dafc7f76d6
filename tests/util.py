"""Shared helpers for the parity tests (thin re-exports so tests read `from util import ...`)."""
import torch as th

from dmesh_renderer_amd.scenes import SUM_ORDER_TOL, sum_order_tol, c_args, elementwise_close, max_abs_err, rel_err, upstream_grads  # noqa: F401

# The background of the tests that run over one: three distinct channels, one negative, one above 1, so that a permutation,
# an abs, a clamp or a sign error of the background terms shows.  (The scenes' own default stays zero: bench.py and the
# golden fixtures use it.)
BG = (0.9, -0.4, 1.7)


def with_bg(d, bg=BG):
    """A copy of the scene dict `d` with the background `bg` (three floats), on the device of d's own."""
    return dict(d, bg=th.tensor(bg, dtype=th.float32, device=d["bg"].device))
