"""Device-code audit of the indexed-mesh translation unit (csrc/surface_mesh.hip), on one compile of its gfx950 ISA, no GPU:
its kernels are the ones listed in tests/golden/device_kernels_surface_mesh.txt (the scan is surface.hip's, whose own list
does not change); every barrier has its LDS drain in front; and no kernel of the unit uses scratch memory -- the emit
kernels index voxels, words and brick offsets by table entries and edge types, which they do in LDS, never in a register
array."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_surface_mesh.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="surface_mesh.hip")


def test_the_mesh_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in ("19k_mesh_vertex_count", "18k_mesh_vertex_emit", "17k_mesh_index_emit"):
        assert sum(name in k for k in got) == 1, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    # vertex count: behind the staging, behind the cubes' liveness, inside the prefix; vertex emit: behind the staging;
    # index emit: behind the staging, inside the prefix
    assert total >= 6
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 3
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
