"""Device-code audit of the slab collider's translation unit (csrc/collide_slab.hip), on one compile of its gfx950 ISA, no
GPU: its kernels are the ones listed in tests/golden/device_kernels_collide_slab.txt (the lists of the other units do not
change with them); every barrier, if there is one, has its LDS drain in front; and each slab collide kernel reads the
wave-uniform triangle record the way the single-domain kernel it mirrors does -- one 16-dword scalar load in the list
walk, two in the indexed walk (the index, and the whole list in a wave with a slow lane) -- with no LDS and no scratch
instruction at all: the broad phase's wave-wide minima and maxima run through DPP moves."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_collide_slab.txt")

# kernel -> (the single-domain kernel it mirrors, that kernel's unit, 16-dword scalar loads)
MIRRORS = {"14k_collide_slabE": ("9k_collideILb1E", "collide.hip", 1),
           "22k_collide_slab_indexedE": ("17k_collide_indexedILb1E", "collide_index.hip", 2)}


@functools.lru_cache(maxsize=None)
def _asm(source="collide_slab.hip"):
    import isa_audit
    return isa_audit.device_asm(source=source)


def _bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN3dsl\w+):", asm, re.M):
        body = asm[m.end():asm.find(".Lfunc_end", m.end())]
        out[m.group(1)] = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith(";")]
    return out


def _x16(body):
    return sum(l.startswith("s_load_dwordx16") for l in body)


def test_the_slab_collider_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert len(got) == 2 and all(any(k in g for g in got) for k in MIRRORS)


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    asm = _asm()
    bad, _total = isa_audit.unprotected_barriers(asm)
    assert not bad, bad
    assert set(re.findall(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", asm)) == {"0"}


def test_the_record_comes_through_scalar_loads_as_in_the_mirrored_kernel_and_nothing_touches_lds_or_scratch():
    bodies = _bodies(_asm())
    seen = 0
    for key, (mirror, unit, loads) in MIRRORS.items():
        (name, body), = [(n, b) for n, b in bodies.items() if key in n]
        (mname, mbody), = [(n, b) for n, b in _bodies(_asm(unit)).items() if mirror in n]
        seen += 1
        assert _x16(mbody) == loads, mname
        assert _x16(body) == loads, name
        assert not any(l.startswith(("ds_", "scratch_")) for l in body), name
        # per particle: the pre-step coordinate, six loads of x and v -- nothing per triangle (the indexed walk adds its
        # cell's bounds and three 16-byte windows of its list)
        assert sum(l.startswith("global_load") for l in body) <= (7 if loads == 1 else 12), name
    assert seen == 2
