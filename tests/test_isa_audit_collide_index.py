"""Device-code audit of the collider index's translation unit (csrc/collide_index.hip), on one compile of its gfx950 ISA,
no GPU: its kernels are the ones listed in tests/golden/device_kernels_collide_index.txt (the lists of dslsph.hip and
collide.hip do not change with them); every barrier, if there is one, has its LDS drain in front; and the indexed collide
kernels read the wave-uniform triangle record with one 16-dword scalar load, as the list walk does."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_collide_index.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="collide_index.hip")


def _bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN3dsl\w+):", asm, re.M):
        body = asm[m.end():asm.find(".Lfunc_end", m.end())]
        out[m.group(1)] = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(";")]
    return out


def test_the_index_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert sum("17k_collide_indexedILb" in k for k in got) == 2


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, _total = isa_audit.unprotected_barriers(_asm())
    assert not bad, bad


def test_the_indexed_kernels_read_the_record_through_one_scalar_load():
    seen = 0
    for name, body in _bodies(_asm()).items():
        if "17k_collide_indexedILb" not in name:
            continue
        seen += 1
        # two walks in the kernel -- over the index, and the whole list in a wave with a slow lane -- one load in each
        assert sum(l.startswith("s_load_dwordx16") for l in body) == 2, name
        assert not any(l.startswith(("ds_read", "ds_write", "scratch_")) for l in body), name
        # the wave-wide minimum of the heads runs in registers: six DPP moves, one readlane, no LDS crossbar
        assert sum("_dpp" in l.split()[0] for l in body) == 6 and not any(l.startswith("ds_bpermute") for l in body), name
        # the cell lists arrive in 16-byte windows: two loads ahead of the walk, one in it
        assert sum(l.startswith("global_load_dwordx4") for l in body) == 3, name
    assert seen == 2
