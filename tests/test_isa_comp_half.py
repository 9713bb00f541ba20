"""The four-quarter strided kernel of the half-domain composition (fft_fixed.hip k_fft_interp_quarters_fx) in the gfx950 code
hipcc emits (cross-compiles without a GPU): no scratch, no spills, and an occupancy no lower than the two-half kernel's
(k_fft_interp_extend_fx) of the same tile."""
import test_isa_properties as isa


def _waves(vgpr):
    """waves per SIMD that a kernel's VGPR count allows on gfx950 (512 registers per lane, allocated in blocks of 8)"""
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


def test_four_quarter_kernel_has_no_scratch_and_the_two_half_kernels_register_tier(tmp_path_factory):
    ks = isa._kernels(isa._emit_asm(tmp_path_factory, "fft_fixed"))
    quarters = isa._find(ks, "k_fft_interp_quarters_fx")
    assert len(quarters) == 4
    for name in quarters:
        body, md = ks[name]
        assert md["vgpr_spill"] == 0 and md["sgpr_spill"] == 0 and "scratch_" not in body, (name, md)
        rb = name[name.index("quarters_fxILi") + len("quarters_fxILi"):].split("E")[0]
        two, = isa._find(ks, "k_fft_interp_extend_fxILi%sE" % rb)
        assert _waves(md["vgpr"]) >= _waves(ks[two][1]["vgpr"]), (name, md, ks[two][1])
