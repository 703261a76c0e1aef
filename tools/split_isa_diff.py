"""Same machine code after a source split: compares the gfx950 device code of two builds kernel by kernel (no GPU needed).

    python tools/split_isa_diff.py PARENT_CSRC [CHILD_CSRC] [-q] [--parent-obj NAME.o ...] [--merged-copies]

PARENT_CSRC / CHILD_CSRC: directories holding the objects of a finished build (`python -m omnifusion_amd.build`), the child's default being
this tree's omnifusion_amd/csrc.  The kernels compared are those of the parent objects named with --parent-obj (repeatable; default
omni_conv_sh.o, the split of the convolution units; the resampling split: --parent-obj omni_equi2pers.o --parent-obj omni_pers2equi.o; the
debug build: the .dbg.o names); on the child side they may live in any object of the same build.

Checked, per kernel: the name exists on both sides, in exactly ONE child object; the instruction sequence is identical (address / encoding
comments stripped, as tests/test_precision_f16x1.py does); the register, LDS and scratch figures of isa.kernel_meta are equal.  The child
units — every object that holds one of these kernels — together hold NO kernel the parent objects together do not.  A kernel that several parent
objects hold (anonymous-namespace kernels of a header that more than one unit compiles) must be in as many child objects, and every parent
copy is matched with a child copy of its own.

--merged-copies (off by default: the rule above is the strict one) is for the change that gives such a header a unit of its own (the
sparse-gather kernels: --parent-obj omni_equi2pers_bwd.o --parent-obj omni_pers2equi_bwd.o, child omni_spgather.o): a kernel that several
parent objects hold may then be in ONE child object, if every parent copy is identical to that copy and to the other parent copies.  Kernels
are then paired by names in which an argument type of the kernel's own anonymous namespace (`NS_7SpApplyE`) reads like a global one (`7SpApply`):
a type that leaves the anonymous namespace because it now crosses units (SpApply, the argument block of those kernels) changes the mangled name
of every kernel that takes it, not its code.  A name that does not pair this way fails the comparison like any missing kernel.

ONE difference is tolerated and printed site by site (-q: a count per kernel): the literal of a pc-relative address formation
    s_getpc_b64 s[n:n+1]; s_add_u32 sn, sn, LIT; s_addc_u32 sn+1, sn+1, LIT
whose target lies OUTSIDE the kernel on both sides — the distance to a symbol of the code object (wino_coef, the GOT slot of omni_sh.h's
sh_overflow_flag), which moves when the kernels around it do.  A formation that lands INSIDE the kernel (a long branch) must match exactly.
Exit status 1 on any other difference.
"""
import argparse
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


def compare(short, pk, pm, ck, cm):
    """([difference], [normalised literal]) between one parent copy and one child copy of a kernel: (start, end, body) and its isa.kernel_meta entry"""
    (ps, pe, pb), (cs, ce, cb) = pk, ck
    bad, notes = [], []
    for key in META:
        if pm.get(key, 0) != cm.get(key, 0):
            bad.append(f"{short}: {key} {pm.get(key, 0)} -> {cm.get(key, 0)}")
    if len(pb) != len(cb):
        return bad + [f"{short}: {len(pb)} instructions -> {len(cb)}"], notes
    psites, csites = external_sites(ps, pe, pb), external_sites(cs, ce, cb)
    both = set(psites) & set(csites)
    for i, ((_, pi), (_, ci)) in enumerate(zip(pb, cb)):
        if pi == ci:
            continue
        site = i if i in both else i - 1 if i - 1 in both else None      # the s_add_u32 of a formation, or the s_addc_u32 behind it
        if site is not None and pi.rsplit(",", 1)[0] == ci.rsplit(",", 1)[0]:
            notes.append(f"  normalised {short}+{pb[i][0] - ps:#x}: `{pi}` -> `{ci}` (targets {psites[site] - ps:+#x} / {csites[site] - cs:+#x} from the kernel's start: outside it)")
            continue
        bad.append(f"{short}+{pb[i][0] - ps:#x}: `{pi}` -> `{ci}`")
        break
    return bad, notes


def global_types(name):
    """the mangled kernel name with every `NS_<length><identifier>E` (a type of the kernel's own anonymous namespace) as `<length><identifier>`"""
    out, i = "", 0
    for m in re.finditer(r"NS_(\d+)", name):
        end = m.end() + int(m.group(1))
        if m.start() >= i and name[end:end + 1] == "E":
            out += name[i:m.start()] + name[m.start() + 3:end]
            i = end + 1
    return out + name[i:]


def copies(objs, merged=False):
    """{kernel name: [(object's base name, (start, end, body), meta)]} over the given objects; merged: the names of --merged-copies"""
    out = collections.OrderedDict()
    for obj in objs:
        meta = {k["name"]: k for k in isa.kernel_meta(obj)}
        ks = kernels(obj)
        keys = [global_types(n) if merged else n for n in ks]
        for key, (n, k) in zip(keys, ks.items()):
            out.setdefault(key, []).append((os.path.basename(obj), k, meta[n]))
    return out


def main():
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("parent_dir")
    ap.add_argument("child_dir", nargs="?", default=os.path.join(ROOT, "omnifusion_amd", "csrc"))
    ap.add_argument("-q", dest="quiet", action="store_true")
    ap.add_argument("--parent-obj", action="append")
    ap.add_argument("--merged-copies", action="store_true")
    opt = ap.parse_args()
    pobjs = opt.parent_obj or ["omni_conv_sh.o"]
    label = " + ".join(pobjs)
    debug = pobjs[0].endswith(".dbg.o")                              # like with like: the debug build's objects, or the product's
    parent = copies([os.path.join(opt.parent_dir, o) for o in pobjs], opt.merged_copies)
    child = copies([o for o in sorted(glob.glob(os.path.join(opt.child_dir, "*.o")))
                    if o.endswith(".dbg.o") == debug and not os.path.basename(o).startswith("omni_debug.")], opt.merged_copies)
    where = {n: [u for u, _, _ in c] for n, c in child.items()}
    bad = []
    units = sorted({u for n in parent for u in where.get(n, [])})
    for u in units:
        for n, w in where.items():
            if u in w and n not in parent:
                bad.append(f"{n}: in the child's units ({', '.join(units)}) but not in the parent's {label}")
    total = nsites = nkernels = 0
    per_unit = collections.Counter()
    for n, pcopies in parent.items():
        # ONE child object per parent object that holds the kernel: exactly one, but for the kernels of a header that several parent objects
        # compile (omni_spgather.h: once per operator), which must be in as many child objects — and every parent copy gets a child copy of its own
        # (--merged-copies: or in ONE child object that every parent copy equals)
        merged = opt.merged_copies and len(pcopies) > 1 and len(where.get(n, [])) == 1
        if len(where.get(n, [])) != len(pcopies) and not merged:
            bad.append(f"{n}: in {len(pcopies)} parent object(s) but {len(where.get(n, []))} child objects {where.get(n, [])}")
            continue
        short = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", n)
        left = list(child[n]) * (len(pcopies) if merged else 1)        # merged: every parent copy against the ONE child copy,
        if merged:                                                     # and the parent copies against each other
            for pname, pk, pm in pcopies[1:]:
                bad += [f"{d} ({pcopies[0][0]} / {pname}: the parent's own copies)" for d in compare(short, pcopies[0][1], pcopies[0][2], pk, pm)[0]]
        for pname, pk, pm in pcopies:
            results = [compare(short, pk, pm, ck, cm) for _, ck, cm in left]
            pick = next((i for i, r in enumerate(results) if not r[0]), 0)
            diffs, notes = results[pick]
            unit = left.pop(pick)[0]
            nkernels += 1
            per_unit[unit] += 1
            total += len(pk[2])
            nsites += len(notes)
            bad += [f"{d} ({pname} -> {unit})" for d in diffs]
            if opt.quiet and notes:
                print(f"  normalised {len(notes):3d} external pc-relative literals in {short}")
            elif notes:
                print("\n".join(notes))
    print(f"{nkernels} kernels, {total} instructions in the parent's {label}; child: " + ", ".join(f"{u} {c}" for u, c in sorted(per_unit.items())))
    print(f"{nsites} literals normalised (pc-relative addresses of symbols outside the kernel), nothing else")
    for b in bad:
        print("DIFFERENT:", b)
    print("split_isa_diff:", "FAILED" if bad else "identical instruction sequences and resource figures for every kernel")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
