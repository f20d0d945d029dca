"""Device-code audit of the recorder's translation unit (csrc/record.hip), on one compile of its gfx950 ISA, no GPU: its kernels
are the ones listed in tests/golden/device_kernels_record.txt; the one barrier -- between the bounds' per-wave results and
their reduction through LDS -- has its LDS drain in front; and no kernel of the unit uses scratch memory: the frame's
description and the id maps travel in the kernel arguments."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_record.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="record.hip")


def test_the_recorder_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name, count in (("15k_record_bounds", 1), ("15k_record_header", 1), ("13k_record_pack", 2)):  # (pack: F32 and Q16)
        assert sum(name in k for k in got) == count, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 1  # the bounds' workgroup reduction
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 4
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)


def test_the_bounds_use_integer_atomics_and_the_division_is_the_correctly_rounded_one():
    """one integer atomic max per key and one add for the count, no compare-and-swap loop; the Q16 scale is the IEEE division
    sequence (scale, fused correction steps, fix-up), not a reciprocal times the numerator"""
    asm = _asm()
    bounds = asm[asm.index("_ZN3dsl15k_record_boundsEiiiNS_5CSoa3ENS_6IdMapsEPj:"):]
    bounds = bounds[:bounds.index("s_endpgm")]
    assert re.search(r"global_atomic_umax\b", bounds) and re.search(r"global_atomic_add\b", bounds) and "cmpswap" not in bounds
    pack = asm[asm.index("_ZN3dsl13k_record_packILb1E"):]
    pack = pack[pack.index(":"):pack.index("s_endpgm")]
    assert pack.count("v_div_fixup_f32") == 3 and pack.count("v_rndne_f32") == 3
