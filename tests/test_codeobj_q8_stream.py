"""The int8-prefilter scan's row stream in the SHIPPED gfx950 code (no GPU needed; tests/codeobj.py).

Every 16-byte row chunk load of `rarc_scan_q8_kernel` is non-temporal (`global_load_dwordx4 ... nt`) and nothing else is:
per instantiation the `nt` loads number exactly CPT (chunks per thread and tile) times the `fetch` sites of its schedule;
the tile metadata pair and the agent-scope threshold / histogram refreshes keep their policy; no scratch, no spill (a
reload in the loop would sit in the queue the counted waits rely on)."""
import re

import pytest

from tests import codeobj

pytestmark = pytest.mark.skipif(not codeobj.os.path.exists(codeobj.LIB), reason="librarc_hip.so not built")

DEEP_D = 384   # Q8_DEEP_D: four fetch groups up to here


def _fetch_sites(d: int, fmt: int) -> int:
    """`fetch` call sites the compiler emits: prologue + one per loop step, the loop copied once per wave group with the
    ping-pong (D <= 768)."""
    ng = 4 if d <= DEEP_D else (2 if fmt else (2 if d <= 896 else 1))
    loops = 2 if d <= 768 else 1
    return {4: 5 + 4 * loops, 2: 3 + 2 * loops, 1: 2 + 2}[ng]


def test_row_chunk_loads_are_non_temporal_and_nothing_else_is():
    dis = codeobj.disassemble("rarc_scan_q8_kernel")
    res = codeobj.kernel_resources()
    seen = set()
    for name, ins in dis.items():
        m = re.search(r"rarc_scan_q8_kernelILi(\d+)ELi(\d)ELi(\d+)E", name)
        assert m, name
        d, fmt, abl = (int(g) for g in m.groups())
        if abl:
            continue
        seen.add((d, fmt))
        cpt = 32 * (d // (16 if fmt else 8)) // 512
        nt = [i for i in ins if re.search(r"\bnt\b", i)]
        assert all(i.startswith("global_load_dwordx4") for i in nt), f"{name}: {[i for i in nt if 'dwordx4' not in i][:3]}"
        assert len(nt) == cpt * _fetch_sites(d, fmt), f"{name}: {len(nt)} nt loads, {cpt} chunks x {_fetch_sites(d, fmt)} fetch sites"
        plain16 = [i for i in ins if i.startswith("global_load_dwordx4") and i not in nt]
        assert len(plain16) >= d // 32, f"{name}: the resident query fragments are {d // 32} plain 16-byte loads"
        assert any(i.startswith("global_load_dwordx2") for i in ins), f"{name}: tile metadata pair"
        assert sum(1 for i in ins if i.startswith("global_load_dword ") and i.endswith("sc1")) >= 2, f"{name}: threshold / histogram refresh"
        r = res[name]
        assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0, (name, r)
    assert {(768, 0), (1024, 1), (768, 2), (128, 0), (384, 0), (1024, 0)} <= seen, seen
