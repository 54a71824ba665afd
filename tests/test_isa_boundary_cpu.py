"""The stream loads' cache policy in the built gfx950 code of libhpgq,
disassembled on the CPU (no GPU), operands kept (tests/test_isa_cpu.py keeps
the mnemonics only).

DESIGN.md §4.1, round 7: the pass-first kernels (single-end stats / filter:
C2, and its N / out-of-range variant) stream their reads with non-temporal
(nt) buffer loads, except -- in C2's kernels -- the LAST step of every group
of steps, which keeps the plain policy: the cache line that step shares with
the next group's first step then stays in L2 until that group's nt load takes
it, instead of coming from HBM twice.  This pins the mixed policy in C2's
kernels (both forms, and no extra load beside them) and round 6's all-nt
policy in the N / out-of-range variant.  The other segmented kernels (edit,
paired-end) re-read lines the stream brought in and keep plain stream loads.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hpg-fastq_amd", "libhpgq.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# engine_tri_kernel<MINW, NM, EDIT, G, FOLLOW> / engine_tri_x_kernel<MINW, NM, G, FOLLOW, XM, EDIT>
C2_HEX = "engine_tri_kernelILi4ELi1ELb0ELi1ELb0EE"
C2_WIDE = "engine_tri_kernelILi4ELi1ELb0ELi2ELb0EE"
C2_TRI = "engine_tri_kernelILi5ELi1ELb0ELi0ELb0EE"
C2_NOOR_HEX = "engine_tri_x_kernelILi4ELi1ELi1ELb0ELi1ELb0EE"
C4_ST = "engine_tri_x_kernelILi4ELi1ELi1ELb0ELi4ELb1EE"      # single-end edit, trims at the step
C3_HEX = "engine_tri_kernelILi3ELi2ELb0ELi1ELb0EE"           # paired-end stats / filter


def _tools():
    return (os.path.exists(LIB) and shutil.which("objcopy")
            and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))
            and os.path.exists(os.path.join(LLVM, "llvm-objdump")))


@pytest.fixture(scope="module")
def loads(tmp_path_factory):
    """{kernel symbol: [(mnemonic, {modifiers})]} of every buffer load of the
    segmented engine kernels, over every gfx950 code object of libhpgq.so."""
    if not _tools():
        pytest.skip("libhpgq.so or the LLVM offload tools are missing")
    d = tmp_path_factory.mktemp("isa_boundary")
    fat = d / "fatbin.bin"
    # (an explicit output file: without one objcopy rewrites its input in place)
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", LIB, str(d / "copy.so")], check=True,
                   capture_output=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = {}
    for i, s in enumerate(starts):
        part = d / f"b{i}.bin"
        part.write_bytes(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = d / f"b{i}.o"
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                            f"--targets={TARGET}", f"--input={part}", f"--output={co}"], capture_output=True)
        if r.returncode or not co.exists() or co.stat().st_size == 0:
            continue
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(co)], check=True,
                             capture_output=True, text=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1) if "engine_tri" in m.group(1) else None
                if cur:
                    out.setdefault(cur, [])
                continue
            m = re.match(r"^\s+(buffer_load_[a-z0-9_]+)\s+([^/]*)", line)
            if cur and m:
                out[cur].append((m.group(1), set(m.group(2).replace(",", " ").split())))
    assert out, "no segmented engine kernel disassembled"
    return out


def _kernel(loads, key):
    hit = [k for k in loads if key in k]
    assert len(hit) == 1, (key, hit)
    return loads[hit[0]]


def _count(ops, mnemonic, nt):
    return sum(1 for op, mods in ops if op == mnemonic and ("nt" in mods) == nt and "lds" not in mods)


@pytest.mark.parametrize("key,stream", [(C2_HEX, "buffer_load_dwordx4"), (C2_WIDE, "buffer_load_dwordx4"),
                                        (C2_TRI, "buffer_load_dwordx2")])
def test_pass_first_kernels_stream_nt_with_a_plain_last_step(loads, key, stream):
    ops = _kernel(loads, key)
    # seq + quality per step at each of at least three load sites (the unit's
    # next group in either slot, the next unit's first group): the last step
    # of a group plain, the step(s) before it nt
    assert _count(ops, stream, True) >= 6, ops
    assert _count(ops, stream, False) >= 6, ops
    # nothing else: every buffer load of the kernel is a stream load
    assert all(op == stream for op, _ in ops), ops


def test_noor_variant_keeps_nt_on_every_step(loads):
    """The N / out-of-range variant is VALU-bound and measured slower with the
    plain last step: it keeps round 6's policy."""
    ops = _kernel(loads, C2_NOOR_HEX)
    assert _count(ops, "buffer_load_dwordx4", True) >= 12, ops
    assert all(op == "buffer_load_dwordx4" and "nt" in mods for op, mods in ops), ops


@pytest.mark.parametrize("key", [C4_ST, C3_HEX])
def test_other_kernels_keep_plain_stream_loads(loads, key):
    ops = _kernel(loads, key)
    assert _count(ops, "buffer_load_dwordx4", False) >= 4, ops
    assert not [o for o in ops if "nt" in o[1]], ops
