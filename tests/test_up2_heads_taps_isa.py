"""CPU, from the built object: the generated code of up2_heads_taps_kernel (csrc/omni_conv_up2_heads_taps.hip) — its register budget (eight waves per block, one
block per CU: 256 registers per lane), no scratch, the 512-thread launch bound, and its matrix instructions, written down:

    per band and wave  2 fragments x 9 taps x 6 (the f16x3 three-term product, K = 32)   = 108
                       2 halves x 2 row segments x 6 (the heads' product with heads.w16f) =  24
                                                                                            132"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "omnifusion_amd", "csrc", "omni_conv_up2_heads_taps.o")
KERNEL = "up2_heads_taps_kernel"
MFMA = 2 * 9 * 6 + 2 * 2 * 6


def _meta():
    from omnifusion_amd import build, isa
    build.build()
    ks = [k for k in isa.kernel_meta(OBJ) if KERNEL in k["name"]]
    assert len(ks) == 1, [k["name"] for k in isa.kernel_meta(OBJ)]
    return ks[0]


def test_register_budget_and_no_scratch():
    k = _meta()
    assert k["vgpr"] + k.get("agpr", 0) <= 256, k
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k
    assert k["lds"] == (36 + 2 * 48) * 1024, k


def test_launch_bound_is_512_threads():
    from omnifusion_amd import build, isa
    import subprocess
    import tempfile
    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        co = isa._device_object(OBJ, tmp)
        notes = subprocess.check_output([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", co]).decode()
    assert notes.count(".name:") and KERNEL in notes
    assert re.findall(r"\.max_flat_workgroup_size:\s*(\d+)", notes) == ["512"]        # the unit's only kernel


def test_matrix_instruction_count_is_pinned():
    from omnifusion_amd import build, isa
    build.build()
    cur, count = None, {}
    for line in isa.disassemble(OBJ).splitlines():
        if line.endswith(">:"):
            cur = line.split("<", 1)[1][:-2]
        elif cur is not None and line.startswith("\t") and line.split("//")[0].strip().startswith("v_mfma"):
            count[cur] = count.get(cur, 0) + 1
    ours = {n: c for n, c in count.items() if KERNEL in n}
    assert list(ours.values()) == [MFMA], count


def test_the_guard_list_names_the_kernel():
    """the build's ISA check (no scratch under hand-placed waits) covers the new kernel"""
    from omnifusion_amd import isa
    assert KERNEL in isa.COUNTED
