"""The aggregation tables of the backward kernels (LDS hash tables in front of the global atomics) fall back to
direct atomics when a row finds no slot.  Real scenes rarely get there, so a child process runs the ABLATION build of
the library (build.py --ablation; the product library has no such switch and ignores the variable) with
DMR_ABLATE set to 2048 -- rows with an odd id are refused a slot -- and checks the gradients against the oracle
(tests/fallback_child.py, started by harness.run_ablation_child)."""
import pytest

from harness import run_ablation_child

pytestmark = pytest.mark.gpu


def test_direct_atomic_fallbacks(hip_device):
    run_ablation_child("default", "fallback ok")
