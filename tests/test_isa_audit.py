"""Device-code audits that need no GPU, on one compile of libdslsph's gfx950 ISA: every s_barrier has the wave's LDS
queue drained (`s_waitcnt lgkmcnt(0)`) in front of it -- see tools/isa_audit.py for the failure this guards against --
and the kernels the host layer instantiates are the ones listed in tests/golden/device_kernels.txt."""
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels.txt")


@functools.lru_cache(maxsize=None)
def _device_asm():
    import isa_audit
    return isa_audit.device_asm()


def test_every_barrier_has_the_lds_queue_drained():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_device_asm())
    assert total > 100  # (the tiled kernels alone hold that many)
    assert not bad, bad[:3]


def test_the_instantiated_kernels_are_the_listed_ones():
    """Which template instantiation of a kernel exists is decided by the launch sites of dslsph.hip (with_flag and the
    `if constexpr` rules beside the launches).  A launch site that names a combination it should not -- or no longer names
    one it should -- changes this list; a kernel added or removed on purpose updates the file in the same commit."""
    import isa_audit
    got = isa_audit.kernel_names(_device_asm())
    want = open(GOLDEN).read().split()
    added, removed = sorted(set(got) - set(want)), sorted(set(want) - set(got))
    dm = isa_audit.demangle(added + removed)
    for what, names in (("added", added), ("removed", removed)):
        for n in names:
            print(f"{what}: {dm[n]}")
    assert not added and not removed, f"{len(added)} kernels added, {len(removed)} removed (names above)"
    assert got == want  # (sorted, no duplicates)
