"""Generates tests/golden/wrapper_{tri,tet}.npz and tests/golden/wrapper_calls.json from a checkout of the
reference project (the one whose `dmesh_renderer/__init__.py` this package mirrors):

    python tests/golden/gen_wrapper_fixtures.py <reference checkout> [--out DIR]

The REFERENCE Python wrapper (<reference checkout>/dmesh_renderer/__init__.py, read-only) is run on
seeded synthetic scenes with `dmesh_renderer._C` provided by tests/oracle_C.py (the CPU oracle), because
the reference's CUDA extension cannot be built without nvcc.  The fixtures therefore pin the Python boundary
(transposes, inverses, dtype casts, gradient routing) and the oracle's numbers on these scenes: the
wrapper's outputs and gradients (npz) and the argument descriptors of every `_C` call it made (json: name,
dtype, shape, stride, contiguity, scalar values).  They are data (inputs are regenerated from the seeds in
tests/test_wrapper_cpu.py), and tests/test_wrapper_cpu.py needs no reference tree to check against them.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_C  # noqa: E402
import test_wrapper_cpu as T  # noqa: E402


def reference_module(ref_root):
    """The reference wrapper, built from its SOURCE TEXT: the file is read, compiled and executed into a fresh module
    object here -- the import machinery is never pointed at the reference tree (no sys.path entry), so its __pycache__
    bytecode is never executed and nothing is written there.  `dmesh_renderer._C` (the unbuilt CUDA extension) is the
    oracle stand-in."""
    path = os.path.join(ref_root, "dmesh_renderer", "__init__.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path} not found: pass the root of a reference checkout")
    saved = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "dmesh_renderer" or k.startswith("dmesh_renderer.")]}
    dont_write = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        with open(path, "r") as f:
            src = f.read()
        mod = types.ModuleType("dmesh_renderer")
        mod.__file__ = path
        mod.__package__ = "dmesh_renderer"
        mod.__path__ = []  # a package with nothing to find: `from . import _C` resolves through sys.modules only
        sys.modules["dmesh_renderer"] = mod
        sys.modules["dmesh_renderer._C"] = oracle_C
        exec(compile(src, path, "exec", dont_inherit=True), mod.__dict__)
        return mod
    finally:
        sys.dont_write_bytecode = dont_write
        for k in [k for k in sys.modules if k == "dmesh_renderer" or k.startswith("dmesh_renderer.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="root of a checkout of the reference project")
    ap.add_argument("--out", default=HERE, help="where the fixtures go (default: tests/golden)")
    a = ap.parse_args()
    ref = reference_module(a.reference)
    os.makedirs(a.out, exist_ok=True)
    calls = {}
    oracle_C.calls.clear()
    c, d, g = T._tri_run(ref, T._tri_scene(), T.TRI["H"], T.TRI["W"])
    calls["tri"] = T.jsonable(oracle_C.calls)
    np.savez_compressed(os.path.join(a.out, "wrapper_tri.npz"), color=c.numpy(), depth=d.numpy(),
                        **{"grad_" + k: v.numpy() for k, v in g.items()})
    oracle_C.calls.clear()
    c, d, a_, g = T._tet_run(ref, T._tet_scene(), T.TET["H"], T.TET["W"])
    calls["tet"] = T.jsonable(oracle_C.calls)
    np.savez_compressed(os.path.join(a.out, "wrapper_tet.npz"), color=c.numpy(), depth=d.numpy(), active=a_.numpy(),
                        **{"grad_" + k: v.numpy() for k, v in g.items()})
    # one argument descriptor per line
    text = ",\n".join(f' "{kind}": [\n' + ",\n".join(f'  ["{name}", [\n' + ",\n".join("   " + json.dumps(x) for x in descs) + "]]"
                                                   for name, descs in calls[kind]) + "]" for kind in calls)
    with open(os.path.join(a.out, "wrapper_calls.json"), "w") as f:
        f.write("{\n" + text + "\n}\n")
    with open(os.path.join(a.out, "wrapper_calls.json")) as f:
        assert json.load(f) == calls
    print("wrote fixtures to", a.out)


if __name__ == "__main__":
    main()
