"""Device-code audit of the collider's translation unit (csrc/collide.hip), on one compile of its gfx950 ISA, no GPU: its
kernels are the ones listed in tests/golden/device_kernels_collide.txt (the engine's own list, device_kernels.txt, is
csrc/dslsph.hip's and does not change with them); they hold no barrier and no LDS; and the collide kernels read the
wave-uniform triangle record with one 16-dword scalar load instead of vector loads."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_collide.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="collide.hip")


def _bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN3dsl\w+):", asm, re.M):
        body = asm[m.end():asm.find(".Lfunc_end", m.end())]
        out[m.group(1)] = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(";")]
    return out


def test_the_collider_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert len(got) == 4


def test_no_barrier_no_lds_and_the_record_comes_through_scalar_loads():
    import isa_audit
    asm = _asm()
    bad, total = isa_audit.unprotected_barriers(asm)
    assert total == 0 and not bad
    assert set(re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", asm)) == {"0"}
    for name, body in _bodies(asm).items():
        if "9k_collideILb" not in name:
            continue
        assert any(l.startswith("s_load_dwordx16") for l in body), name
        assert not any(l.startswith(("ds_read", "ds_write", "scratch_")) for l in body), name
        # per particle: six loads of x and v, the boundary test's id -- nothing per triangle
        assert sum(l.startswith("global_load") for l in body) <= 8, name
