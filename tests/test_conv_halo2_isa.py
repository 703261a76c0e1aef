"""CPU: the generated code of halo2_sh_kernel (omni_conv_halo2.hip).  Two blocks per CU need at most 256 registers per wave (architectural and
accumulation registers together) and at most 80 KiB of LDS per block; a spill inside the K loop would be a performance bug (isa.HOT)."""
import os


def test_halo2_kernels_fit_two_blocks_per_cu_without_scratch():
    from omnifusion_amd import build, isa
    build.build()
    assert isa.check() == []
    assert "halo2_sh_kernel" in isa.HOT
    obj = os.path.join(build.CSRC, "omni_conv_halo2.o")
    rows = [r for r in isa.table([obj]) if "halo2_sh_kernel" in r[1]]
    assert len(rows) == 4, rows                                   # IW 0 | 16, f16x3 | f16x1 (the names may come mangled)
    for _, name, vgpr, agpr, _, lds, scratch in rows:
        assert scratch == 0, (name, scratch)
        assert vgpr + agpr <= 256, (name, vgpr, agpr)
        assert lds <= 80 * 1024, (name, lds)
