"""Static check of the compiled kernels for the gfx950 wide-store data hazard (tools/probes/storewar_probe.hip):
a vector store of more than 8 bytes reads its data VGPRs a few clocks after it issues, so nothing may write one of them in the next
two issue slots.  LLVM inserts one wait state, and none when the store has an SGPR scalar offset; the fused temporal self-attention
kernel lost elements of its saved `o` that way.  This test compiles every HIP source of the library to ISA (no GPU needed) and walks
the fall-through path behind every `*_store_dwordx3/x4`."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svd_xtend_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def scan(asm_text, need=2):
    """-> list of (wait states seen, store line, overwriting line) for wide stores whose data register is written again before `need`
    wait states have passed (straight-line code only: a branch ends the window)."""
    lines = [ln.strip() for ln in asm_text.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith((";", ".", "//"))]
    hits = []
    for i, ln in enumerate(lines):
        m = re.match(r"((?:buffer|global|flat|scratch)_store_dwordx[34])\s+(.*)", ln)
        if not m:
            continue
        ops = [o.strip() for o in m.group(2).split(",")]
        data = _regs(ops[0] if m.group(1).startswith("buffer") else ops[1])
        gap = 0
        for nxt in lines[i + 1:i + 1 + need + 2]:
            if gap >= need:
                break
            op = nxt.split()[0]
            if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
                break
            if op.startswith(("v_", "ds_read", "buffer_load", "global_load", "flat_load")) and " " in nxt:
                if _regs(nxt.split(None, 1)[1].split(",")[0].strip()) & data:
                    hits.append((gap, ln, nxt))
                    break
            gap += int(nxt.split()[1]) + 1 if op == "s_nop" else 1
    return hits


def test_scanner_sees_the_pattern():
    bad = "buffer_store_dwordx4 v[12:15], v72, s[16:19], s26 offen\nv_xor_b32_e32 v12, s0, v164\n"
    one = "buffer_store_dwordx4 v[12:15], v72, s[16:19], 0 offen\ns_nop 0\nv_mov_b32_e32 v13, 0\n"
    ok = "buffer_store_dwordx4 v[12:15], v72, s[16:19], 0 offen\ns_nop 1\nv_mov_b32_e32 v13, 0\n"
    other = "global_store_dwordx4 v[2:3], v[12:15], off\nv_mov_b32_e32 v2, 0\nv_mov_b32_e32 v16, 0\n"     # the ADDRESS may be reused
    assert len(scan(bad)) == 1 and len(scan(one)) == 1 and not scan(ok) and not scan(other)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_wide_store_has_its_data_overwritten_within_two_wait_states(tmp_path):
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))

    def compile_one(src):
        out = str(tmp_path / (src + ".s"))
        r = subprocess.run([HIPCC, "-w", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                            os.path.join(CSRC, src), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return src, open(out).read()

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        texts = list(ex.map(compile_one, srcs))
    total_stores, report = 0, []
    for src, txt in texts:
        total_stores += len(re.findall(r"_store_dwordx[34]\s", txt))
        report += [(src,) + h for h in scan(txt)]
    assert total_stores > 1000                       # the scan saw the library (the three gemm_*.hip units alone have ~600 wide stores)
    assert not report, report[:10]
