"""Compile resources and instruction lines of every kernel in `hipcc --cuda-device-only -S` listings, one side against another.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -S --cuda-device-only -o parent/dmr_shade.s ...
    python scripts/kernel_resources.py [--rename OLD=NEW ...] parent/dmr_shade.s branch/dmr_shade.s [parent/dmr_texture.s branch/dmr_texture.s ...]

--rename OLD=NEW: a kernel the first side calls OLD is compared with the second side's NEW.

Per kernel and side: VGPR AGPR SGPR scratch(bytes/lane) VGPR-spill SGPR-spill LDS(bytes/block) occupancy(waves/SIMD) | instruction
lines (every line of the body that is no directive, comments stripped, labels included), and whether the bodies are the same
line for line.  Exit status 1 when a kernel of the second side has scratch, a VGPR spill, another LDS size or occupancy, or
more SGPR spills than the first side's.
"""
import re
import subprocess
import sys


def kernels(path):
    """{demangled name: (columns, body lines)}"""
    text = open(path).read()
    spills = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(
        r"\.name:\s+(_Z\w+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s*(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s*(\d+)", text)}
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; Occupancy: (\d+)", text, re.S | re.M):
        sym, body, tail, occ = m.group(1), m.group(2), m.group(3), int(m.group(4))
        if sym not in spills:
            continue
        get = lambda key: int(re.search(key + r":? (\d+)", tail).group(1))
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in body.split("\n")]  # (less the function's ordinal in its file)
        lines = [l for l in lines if l and not l.startswith(".") or l.endswith(":")]
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^(?:void )?(?:dmr::)?(?:\(anonymous namespace\)::)?", "", name).split("(")[0]  # (a return type: templates alone)
        out[name] = ((get("NumVgprs"), get("NumAgprs"), get("NumSgprs"), get("ScratchSize"), spills[sym][1], spills[sym][0],
                      get("LDSByteSize"), occ), lines)
    return out


def main(args):
    bad = 0
    renames, paths = {}, []
    while args:
        if args[0] == "--rename":
            old, new = args[1].split("=")
            renames[old] = new
            args = args[2:]
        else:
            paths.append(args[0])
            args = args[1:]
    for a, b in zip(paths[::2], paths[1::2]):
        ka, kb = kernels(a), kernels(b)
        ka = {renames.get(name, name): v for name, v in ka.items()}
        unit = a.split("/")[-1].split(".")[0]
        for name in ka:
            (ca, la), (cb, lb) = ka[name], kb[name]
            ok = cb[3] == 0 and cb[4] == 0 and cb[6] == ca[6] and cb[7] == ca[7] and cb[5] <= ca[5]
            bad += not ok
            fmt = lambda c, n: "".join(f"{x:7d}" for x in c) + f" | {n:6d}"
            print(f"{unit:12s} {name:52s} parent {fmt(ca, len(la))}")
            print(f"{'':12s} {'':52s} branch {fmt(cb, len(lb))}  {'same' if la == lb else 'differs'}{'' if ok else '  CONDITION MISSED'}")
        assert sorted(ka) == sorted(kb), (sorted(ka), sorted(kb))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
