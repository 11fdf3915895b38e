"""The int8-prefilter scan's tile loop in the SHIPPED gfx950 code with the threshold / histogram refresh once per loop unit at
every D (no GPU needed; tests/codeobj.py).  The tile's metadata pair stays a vector load (its scalar form was measured slower:
DESIGN.md 4.1).

Per instantiation: no scratch, no spilled VGPR, at most 256 VGPRs; the 16-byte non-temporal row loads number what they did in the
parent commit's code object (PARENT_NT, read from it: chunks per thread x fetch sites); and the tile loop — the innermost
loop that holds the MFMAs, one copy per wave group up to D = 768 — issues fewer vector-memory loads per trip than the
parent's above 384 dimensions (PARENT_LOOP_LOADS, read from the parent's code object the same way: a trip is one unit, two
tiles, four up to 384 dimensions, where the parent refreshed once per unit already and the count is the parent's), every one of
the difference a load that carried no row bytes: the row loads per trip are unchanged."""
import re

import pytest

from tests import codeobj

pytestmark = pytest.mark.skipif(not codeobj.os.path.exists(codeobj.LIB), reason="librarc_hip.so not built")

# (D, FMT) -> 16-byte `nt` loads in the whole kernel, parent commit
PARENT_NT = {(128, 0): 13, (256, 0): 26, (384, 0): 39, (512, 0): 28, (640, 0): 35, (768, 0): 42, (896, 0): 35, (1024, 0): 32,
             (256, 1): 13, (512, 1): 14, (768, 1): 21, (1024, 1): 20, (256, 2): 13, (512, 2): 14, (768, 2): 21, (1024, 2): 20}
# (D, FMT) -> vector-memory loads per trip of each tile loop, parent commit: row chunks + (pair, threshold, histogram word) per
# tile; with four fetch groups the parent refreshed in one group of four already (fp8 rows: + the rows' multipliers)
PARENT_LOOP_LOADS = {(128, 0): 10, (256, 0): 14, (384, 0): 18, (512, 0): 14, (640, 0): 16, (768, 0): 18, (896, 0): 20,
                     (1024, 0): 22, (256, 1): 14, (512, 1): 14, (768, 1): 18, (1024, 1): 22, (256, 2): 10, (512, 2): 10,
                     (768, 2): 12, (1024, 2): 14}


def _instantiations():
    for name, listing in codeobj.disassemble_addr("rarc_scan_q8_kernel").items():
        m = re.search(r"rarc_scan_q8_kernelILi(\d+)ELi(\d)ELi(\d+)E", name)
        assert m, name
        d, fmt, abl = (int(g) for g in m.groups())
        if abl == 0:
            yield name, d, fmt, listing


def _tile_loops(listing, unit):
    """The tile loops, [instruction texts] each: the backward branches whose range holds one unit of tiles — the fewest MFMAs
    of any loop with MFMAs in it, and `unit` barriers (the loop over ranges around it holds the prologue's barrier as well).
    A loop the compiler rotated has several such branches; overlapping ranges are one loop."""
    index_of = {a: i for i, (a, _) in enumerate(listing)}
    edges = []
    for i, (addr, text) in enumerate(listing):
        if not text.startswith(("s_cbranch", "s_branch")):
            continue
        j = index_of.get(codeobj._branch_target(addr, text))
        if j is not None and j <= i:
            body = [t for _, t in listing[j:i + 1]]
            n = sum(1 for t in body if t.startswith("v_mfma"))
            if n:
                edges.append((j, i, n, sum(1 for t in body if t.startswith("s_barrier"))))
    fewest = min(n for _, _, n, _ in edges)
    spans = []
    for a, b, n, bars in sorted(edges):
        if n != fewest or bars > unit:
            continue
        if spans and a <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    return [[t for _, t in listing[a:b + 1]] for a, b in spans]


def _is_vmem_load(t):
    return t.startswith(("global_load", "flat_load", "buffer_load"))


def test_no_scratch_no_spill_256_vgprs():
    res = codeobj.kernel_resources()
    seen = set()
    for name, d, fmt, _ in _instantiations():
        r = res[name]
        seen.add((d, fmt))
        assert r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, (name, r)
    assert seen == set(PARENT_NT), seen ^ set(PARENT_NT)


def test_row_loads_unchanged():
    for name, d, fmt, listing in _instantiations():
        nt = [t for _, t in listing if re.search(r"\bnt\b", t)]
        assert all(t.startswith("global_load_dwordx4") for t in nt), name
        assert len(nt) == PARENT_NT[(d, fmt)], f"{name}: {len(nt)} non-temporal 16-byte loads, the parent has {PARENT_NT[(d, fmt)]}"


def test_tile_loop_issues_fewer_vector_memory_loads():
    for name, d, fmt, listing in _instantiations():
        ng = 4 if d <= 384 else 2
        loops = _tile_loops(listing, ng)
        assert len(loops) == (2 if d <= 768 else 1), f"{name}: {len(loops)} tile loops (one per wave group with the ping-pong)"
        cpt = 32 * (d // (16 if fmt else 8)) // 512
        for ins in loops:
            loads = [t for t in ins if _is_vmem_load(t)]
            rows = [t for t in loads if re.search(r"\bnt\b", t)]
            assert sum(1 for t in ins if t.startswith("s_barrier")) == ng, name
            assert len(rows) == ng * cpt, f"{name}: {len(rows)} row loads per trip, {ng} tiles x {cpt} chunks"
            parent = PARENT_LOOP_LOADS[(d, fmt)]
            assert (len(loads) < parent) if d > 384 else (len(loads) == parent), \
                f"{name}: {len(loads)} vector-memory loads per trip, the parent has {parent}"
            # what is left besides the rows: a metadata pair per tile, one threshold and one histogram word per trip (fp8: + a
            # multiplier per chunk)
            assert len(loads) - len(rows) == ng + 2 + (ng * cpt if fmt == 1 else 0), f"{name}: {[t for t in loads if t not in rows]}"
            assert sum(1 for t in ins if t.startswith("global_load_dwordx2")) == ng, name
            assert sum(1 for t in ins if t.startswith("global_load_dword ") and t.endswith("sc1")) == 2, name


def test_headline_loop_against_parent():
    """D = 768 fp16 rows, per iteration pair: 18 vector-memory loads in the parent (12 row chunks, 2 pairs, 2 thresholds, 2
    histogram words), 16 now (12 row chunks, 2 pairs, one threshold, one histogram word)."""
    (listing,) = [l for _, d, fmt, l in _instantiations() if (d, fmt) == (768, 0)]
    for ins in _tile_loops(listing, 2):
        assert sum(1 for t in ins if _is_vmem_load(t)) == 16 < PARENT_LOOP_LOADS[(768, 0)]
