"""Same machine code after a source split: compares the gfx950 device code of two builds kernel by kernel (no GPU needed).

    python tools/split_isa_diff.py PARENT_CSRC [CHILD_CSRC] [-q]

PARENT_CSRC / CHILD_CSRC: directories holding the objects of a finished build (`python -m omnifusion_amd.build`), the child's default being
this tree's omnifusion_amd/csrc.  The kernels compared are those of the parent's omni_conv_sh.o; on the child side they may live in any object.

Checked, per kernel: the name exists on both sides, in exactly ONE child object; the instruction sequence is identical (address / encoding
comments stripped, as tests/test_precision_f16x1.py does); the register, LDS and scratch figures of isa.kernel_meta are equal.

ONE difference is tolerated and printed site by site (-q: a count per kernel): the literal of a pc-relative address formation
    s_getpc_b64 s[n:n+1]; s_add_u32 sn, sn, LIT; s_addc_u32 sn+1, sn+1, LIT
whose target lies OUTSIDE the kernel on both sides — the distance to a symbol of the code object (wino_coef, the GOT slot of omni_sh.h's
sh_overflow_flag), which moves when the kernels around it do.  A formation that lands INSIDE the kernel (a long branch) must match exactly.
Exit status 1 on any other difference.
"""
import collections
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omnifusion_amd import isa  # noqa: E402

META = ("vgpr", "agpr", "sgpr", "lds", "scratch", "vgpr_spill", "sgpr_spill")


def kernels(obj):
    """{name: (start address, end address, [(address, instruction)])} of one object's device code; kernels only."""
    names = {k["name"] for k in isa.kernel_meta(obj)}
    out, cur = collections.OrderedDict(), None
    for line in isa.disassemble(obj).splitlines():
        if line.endswith(">:"):
            cur = line.split("<", 1)[1][:-2]
            addr = int(line.split()[0], 16)
            for v in out.values():
                if v[1] is None:
                    v[1] = addr
            out[cur] = [addr, None, []]
        elif cur and line.startswith("\t"):
            ins, _, tail = line.partition("//")
            ins = ins.strip()
            if ins and ins != "...":
                out[cur][2].append((int(tail.split(":")[0], 16), ins))
    for v in out.values():
        if v[1] is None:
            v[1] = v[2][-1][0] + 8 if v[2] else v[0]
    return {n: tuple(v) for n, v in out.items() if n in names}


def external_sites(start, end, body):
    """{index of the s_add_u32: target} for every pc-relative address formation of `body` whose target is outside [start, end)."""
    sites = {}
    for i in range(len(body) - 2):
        g = re.fullmatch(r"s_getpc_b64 s\[(\d+):(\d+)\]", body[i][1])
        if not g:
            continue
        lo, hi = g.group(1), g.group(2)
        a = re.fullmatch(rf"s_add_u32 s{lo}, s{lo}, (0x[0-9a-f]+|-?\d+)", body[i + 1][1])
        c = re.fullmatch(rf"s_addc_u32 s{hi}, s{hi}, (0x[0-9a-f]+|-?\d+)", body[i + 2][1])
        if not (a and c):
            continue
        off = (int(a.group(1), 0) & 0xffffffff) | ((int(c.group(1), 0) & 0xffffffff) << 32)
        if off >= 1 << 63:
            off -= 1 << 64
        target = body[i][0] + 4 + off                               # s_getpc_b64 returns the address of the NEXT instruction
        if not (start <= target < end):
            sites[i + 1] = target
    return sites


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    quiet = "-q" in sys.argv
    if not args:
        sys.exit(__doc__)
    parent_dir = args[0]
    child_dir = args[1] if len(args) > 1 else os.path.join(ROOT, "omnifusion_amd", "csrc")
    pobj = os.path.join(parent_dir, "omni_conv_sh.o")
    parent = kernels(pobj)
    pmeta = {k["name"]: k for k in isa.kernel_meta(pobj)}
    child, cmeta, where = {}, {}, collections.defaultdict(list)
    for obj in sorted(glob.glob(os.path.join(child_dir, "*.o"))):
        if obj.endswith(".dbg.o") or os.path.basename(obj) == "omni_debug.o":
            continue
        ks = kernels(obj)
        for n in ks:
            where[n].append(os.path.basename(obj))
        child.update(ks)
        cmeta.update({k["name"]: k for k in isa.kernel_meta(obj)})
    bad = []
    for n in parent:
        if len(where[n]) != 1:
            bad.append(f"{n}: in {len(where[n])} child objects {where[n]}")
    units = sorted({w for n in parent for w in where[n]})
    extra = [n for u in units for n, w in where.items() if u in w and n not in parent]
    for n in extra:
        bad.append(f"{n}: in the child's conv units but not in the parent's omni_conv_sh.o")
    total = nsites = 0
    per_unit = collections.Counter()
    for n, (ps, pe, pb) in parent.items():
        if len(where[n]) != 1:
            continue
        cs, ce, cb = child[n]
        per_unit[where[n][0]] += 1
        total += len(pb)
        short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", n)
        for key in META:
            if pmeta[n].get(key, 0) != cmeta[n].get(key, 0):
                bad.append(f"{short}: {key} {pmeta[n].get(key, 0)} -> {cmeta[n].get(key, 0)}")
        if len(pb) != len(cb):
            bad.append(f"{short}: {len(pb)} instructions -> {len(cb)}")
            continue
        psites, csites = external_sites(ps, pe, pb), external_sites(cs, ce, cb)
        both = set(psites) & set(csites)
        count = 0
        for i, ((_, pi), (_, ci)) in enumerate(zip(pb, cb)):
            if pi == ci:
                continue
            site = i if i in both else i - 1 if i - 1 in both else None      # the s_add_u32 of a formation, or the s_addc_u32 behind it
            if site is not None and pi.rsplit(",", 1)[0] == ci.rsplit(",", 1)[0]:
                count += 1
                if not quiet:
                    print(f"  normalised {short}+{pb[i][0] - ps:#x}: `{pi}` -> `{ci}` (targets {psites[site] - ps:+#x} / {csites[site] - cs:+#x} from the kernel's start: outside it)")
                continue
            bad.append(f"{short}+{pb[i][0] - ps:#x}: `{pi}` -> `{ci}`")
            break
        nsites += count
        if quiet and count:
            print(f"  normalised {count:3d} external pc-relative literals in {short}")
    print(f"{len(parent)} kernels, {total} instructions in the parent's omni_conv_sh.o; child: " + ", ".join(f"{u} {c}" for u, c in sorted(per_unit.items())))
    print(f"{nsites} literals normalised (pc-relative addresses of symbols outside the kernel), nothing else")
    for b in bad:
        print("DIFFERENT:", b)
    print("split_isa_diff:", "FAILED" if bad else "identical instruction sequences and resource figures for every kernel")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
