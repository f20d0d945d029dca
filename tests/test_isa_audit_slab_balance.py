"""Device-code audit of the slab re-balancing count's translation unit (csrc/slab_balance.hip), on one compile of its
gfx950 ISA, no GPU: its kernels are the ones listed in tests/golden/device_kernels_slab_balance.txt (the lists of
dslsph.hip, collide.hip and collide_index.hip do not change with it), and every barrier has its LDS drain in front."""
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_slab_balance.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="slab_balance.hip")


def test_the_balance_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert sum("18k_slab_layer_count" in k for k in got) == 1


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 2  # the histogram is cleared before, and complete before it is flushed
    assert not bad, bad


def test_the_unit_is_built_into_the_library():
    from dieselfluid_amd import _lib
    assert "slab_balance.hip" in _lib.UNITS
