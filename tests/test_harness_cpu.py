"""tests/harness.py without a GPU: the cases the GPU tests hand to the child launchers exist, and a child that outlives
its time limit is ended together with everything it started."""
import glob
import os
import re
import sys
import time

import pytest

import harness

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_launched_case_exists():
    """A typo in a case name (or in the line a child prints) would otherwise only show on the GPU box."""
    import fallback_child
    import sharded_child
    known = {"run_ranks": sharded_child.CASES, "run_ablation_child": fallback_child.CASES}
    used = {fn: set() for fn in known}
    for path in glob.glob(os.path.join(HERE, "test_*_gpu.py")):
        with open(path) as f:
            for fn, case, ok_line in re.findall(r'\b(run_ranks|run_ablation_child)\("(\w+)", "([^"]+)"\)', f.read()):
                assert case in known[fn] and known[fn][case][1] == ok_line, (path, fn, case, ok_line)
                used[fn].add(case)
    assert used == {fn: set(cases) for fn, cases in known.items()}  # and no case that no test runs


def _gone(pid):
    try:
        with open(f"/proc/{pid}/stat") as f:
            return f.read().rsplit(")", 1)[1].split()[0] == "Z"  # killed, not yet reaped by init
    except FileNotFoundError:
        return True


def test_time_out_ends_the_whole_process_group(tmp_path):
    """The launcher's time-out path on host processes: a child that starts a grandchild, ignores TERM and sleeps."""
    pids = tmp_path / "pids"
    script = ("import os, signal, subprocess, sys, time\n"
              "signal.signal(signal.SIGTERM, signal.SIG_IGN)\n"
              "g = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(600)'])\n"
              f"open({str(pids)!r}, 'w').write(f'{{os.getpid()}} {{g.pid}}')\n"
              "print('started', flush=True)\n"
              "time.sleep(600)\n")
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match=r"timed out after 2 s(.|\n)*started"):
        harness._run_child([sys.executable, "-c", script], "never printed", timeout=2, grace=1)
    assert time.monotonic() - t0 < 30
    child, grandchild = (int(x) for x in pids.read_text().split())
    deadline = time.monotonic() + 10
    while not (_gone(child) and _gone(grandchild)) and time.monotonic() < deadline:
        time.sleep(0.05)
    assert _gone(child) and _gone(grandchild)
