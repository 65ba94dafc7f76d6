"""Do two builds of libdmesh_renderer_hip.so compute the same bits in the fused shading units?

    python scripts/shading_bits.py parent=<path to one build> branch=<path to another>

For each library a fresh child process (this script with --dump, DMR_LIBRARY=<path>, under its own time limit; the first that
fails ends the run) runs, over every call of tests/shading_cases.tables(), the unit's forward and its backward for dL/dbary
alone, on seeded inputs, and writes the SHA-256 of image, T and dL/dbary: what has one writer per element and no atomics (the
other gradients go through float atomics and are not comparable bit for bit).  Then the digests are compared; exit status 1
when any differs.  Lists: random face ids with empty slots anywhere, opacities that include 0 and 1, barycentrics in the face.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME, F, P, TEXTURE = (2, 24, 40), 600, 900, (7, 13)


def dump(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch as th
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    assert _C.library_path() == os.environ["DMR_LIBRARY"], _C.library_path()
    dev = th.device("cuda:0")
    digest = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    res = {}
    for table, rows in SC.tables().items():
        for i, r in enumerate(rows):
            g = th.Generator().manual_seed(1000 + len(res))
            B, H, W = FRAME
            rnd = lambda *s: th.rand(*s, generator=g)
            face = th.randint(-1, F, (B, r.K, H, W), generator=g).to(th.int32)
            u = rnd(B, r.K, 1, H, W)
            bary = th.cat([u, (1 - u) * rnd(B, r.K, 1, H, W)], 2)
            opacity = rnd(F)
            opacity[::7], opacity[3::11] = 0.0, 1.0
            scale = 0.5 + rnd(B, F)
            gi, gt = th.randn(B, r.C, H, W, generator=g), th.randn(B, 1, H, W, generator=g)
            place = (lambda t: t.to(dev)) if r.aligned else (lambda t: SC.one_float_in(t.to(dev)))
            if r.unit == "shade":
                corners = th.randint(0, P, (F, 3), generator=g).to(th.int32)
                own = [place(th.randn(P, r.C, generator=g))]
                tail, fwd, need = [], _C.composite_fragments, (False, False, False, True)
            else:
                corners = th.randint(0, P, (F, 3), generator=g).to(th.int32)
                own = [rnd(P, 2).to(dev), place(th.randn(*TEXTURE, r.C, generator=g))]
                tail, fwd, need = [1], _C.composite_texture, (False, False, bool(r.tex), False, True)
            assert own[-1].data_ptr() % 16 == (0 if r.aligned else 4)
            args = [face.to(dev), bary.to(dev), corners.to(dev), opacity.to(dev)] + own + [scale.to(dev)] + tail
            image, T = fwd(*args)
            bwd = _C.composite_fragments_backward if r.unit == "shade" else _C.composite_texture_backward
            dbary = bwd(*args, gi.to(dev), gt.to(dev), need)[-1]
            th.cuda.synchronize()
            res[f"{table}[{i}] {tuple(r)}"] = {"image": digest(image), "T": digest(T), "dL_dbary": digest(dbary)}
    json.dump(res, open(out, "w"), indent=1)


def main(argv):
    if argv[0] == "--dump":
        return dump(argv[1])
    sides = {}
    with tempfile.TemporaryDirectory() as tmp:
        for arg in argv:
            name, path = arg.split("=", 1)
            out = os.path.join(tmp, name + ".json")
            env = dict(os.environ, DMR_LIBRARY=os.path.abspath(path))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", out], env=env, check=True, timeout=300)
            sides[name] = json.load(open(out))
    (a, da), (b, db) = sides.items()
    assert sorted(da) == sorted(db)
    differ = [(k, o) for k in da for o in da[k] if da[k][o] != db[k][o]]
    print(f"# {a} against {b}: {len(da)} calls of shading_cases.tables(), image, T and dL/dbary of each: {3 * len(da)} digests")
    for k in da:
        same = [o for o in da[k] if da[k][o] == db[k][o]]
        print(f"{k:70s} {'same' if len(same) == 3 else 'DIFFERS in ' + ', '.join(o for o in da[k] if o not in same)}  {da[k]['image'][:12]}")
    print(f"# differing: {len(differ)}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
