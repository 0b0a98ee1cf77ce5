"""Build hygiene of the shipped library (runs on CPU: hipcc cross-compiles gfx950 without a GPU).

* no MFMA kernel instantiation spills (round-1 finding: spilling variants compiled into the product);
* the library reads no environment variable (round-1 finding: test knobs steering the product at run time);
* every symbol of include/avcer_hip.h is exported (also checked by __graft_entry__.build)."""
import os
import re
import shutil
import subprocess

import pytest

from avcer_amd import _lib, build

CSRC = build.CSRC


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("hipcc not available")
    return exe


_ASM_CACHE = {}


def _device_asm(src):
    """The device ISA of one source file, compiled once per test session (three tests read fused.hip's, two gemm.hip's)."""
    if src not in _ASM_CACHE:
        import tempfile

        out = os.path.join(tempfile.mkdtemp(prefix="avcer_asm_"), src + ".s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
        r = subprocess.run([_hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        _ASM_CACHE[src] = out
    return _ASM_CACHE[src]


@pytest.mark.parametrize("src", ["gemm.hip", "fused.hip"])
def test_mfma_kernels_do_not_spill(src):
    """No kernel of the two MFMA sources may use scratch memory or spill a register (the code object's own metadata)."""
    txt = open(_device_asm(src)).read()
    kernels = re.findall(r"- \.agpr_count:.*?\.wavefront_size", txt, re.S)
    assert len(kernels) >= 10
    bad = []
    for k in kernels:
        g = lambda key: re.search(r"\." + key + r":\s+(\S+)", k).group(1)
        if int(g("private_segment_fixed_size")) or int(g("vgpr_spill_count")) or int(g("sgpr_spill_count")):
            bad.append((g("name"), g("private_segment_fixed_size"), g("vgpr_spill_count"), g("sgpr_spill_count")))
    assert not bad, bad


def test_library_reads_no_environment_and_exports_the_header():
    lib = build.build()
    und = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True).stdout
    assert "getenv" not in und
    defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    header = open(os.path.join(CSRC, "..", "..", "include", "avcer_hip.h")).read()
    declared = set(re.findall(r"\b(avcer_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert re.search(rf"\b{name}\b", defined), name


def _audit_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("audit_asm_loads", os.path.join(os.path.dirname(CSRC), "..", "tools", "audit_asm_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("src,kernel,instances", [("fused.hip", "bneck_tail2_kernel", 1), ("gemm.hip", "conv_gemm_wd_kernel", 16),
                                                 ("fused.hip", "ELb0ELi1ELb1EE", 2)])  # the two T11 instantiations of bneck_kernel
def test_asm_loaded_registers_are_untouched_until_their_wait(src, kernel, instances, tmp_path):
    """Every kernel that loads into VGPRs by inline asm (the residual ring of bneck_tail2_kernel, the weight fragments of all
    sixteen conv_gemm_wd_kernel instantiations and of the two spatial-tile (T11) forms of bneck_kernel): only the kernel's counted `s_waitcnt vmcnt(N)` protects those registers, so
    tools/audit_asm_loads.py walks the generated ISA's control-flow graph with the queue of outstanding vector-memory
    operations as its state and checks that no instruction reads or writes a register with an asm load in flight."""
    asm = _device_asm(src)
    mod = _audit_module()
    assert len(mod.kernels(asm, kernel)) == instances
    assert mod.audit(asm, kernel) == []


def _store_data_hazards(asm_text):
    """(kernel, store, next instruction) wherever a 12- / 16-byte buffer store is followed at once by a VALU write of one of its
    data registers."""
    bad, kernel, prev = [], "?", None
    for line in asm_text.splitlines():
        t = line.strip()
        if not t or t.startswith((";", ".")):
            continue
        if t.endswith(":") and not t.startswith(".L"):
            kernel, prev = t[:-1], None
            continue
        if prev is not None and t.startswith("v_"):
            m = re.match(r"v_\w+\s+(v\[(\d+):(\d+)\]|v(\d+))", t)
            if m:
                lo, hi = (int(m.group(2)), int(m.group(3))) if m.group(2) else (int(m.group(4)), int(m.group(4)))
                if lo <= prev[1] and hi >= prev[0]:
                    bad.append((kernel, prev[2], t))
        prev = None
        m = re.match(r"buffer_store_dwordx[34]\s+v\[(\d+):(\d+)\]", t)
        if m:
            prev = (int(m.group(1)), int(m.group(2)), t)
    return bad


@pytest.mark.parametrize("src", ["fused.hip", "gemm.hip", "kernels.hip", "detect_tail.hip"])
def test_no_valu_write_right_behind_a_wide_buffer_store(src, tmp_path):
    """gfx950 reads the data registers of a 16-byte buffer store a moment after issue, and hipcc only separates a following VALU
    write of them by a wait state when the store's scalar offset is a constant ("this hazard only exists if the instruction is
    not using a register in the soffset field"): with the offset in an SGPR it emitted `v_max3_f32 v0, ..` right behind
    `buffer_store_dwordx4 v[0:3], ..` in a lab form of the chain kernels, and 4 lanes x 1 dword of the stored rows changed from
    run to run (profiles/experiments/README.md, round 5).  No shipped kernel may contain that pair."""
    assert _store_data_hazards(open(_device_asm(src)).read()) == []


def test_the_store_data_hazard_scan_sees_the_pair():
    hazard = "_Z1kv:\nbuffer_store_dwordx4 v[0:3], v80, s[4:7], s16 offen\nv_max3_f32 v0, v89, |v8|, |v9|\ns_endpgm\n"
    assert len(_store_data_hazards(hazard)) == 1
    fine = "_Z1kv:\nbuffer_store_dwordx4 v[0:3], v80, s[4:7], s16 offen\ns_nop 0\nv_max3_f32 v0, v89, |v8|, |v9|\ns_endpgm\n"
    assert _store_data_hazards(fine) == []
    other = "_Z1kv:\nbuffer_store_dwordx4 v[0:3], v80, s[4:7], s16 offen\nv_max3_f32 v4, v0, |v8|, |v9|\ns_endpgm\n"
    assert _store_data_hazards(other) == []


def test_the_asm_load_audit_catches_a_hazard(tmp_path):
    """The audit on hand-written ISA: a use before the counted wait, a use on a path that skips the wait, an overwrite of
    the destination and a missing drain are reported; the correct sequences are not."""
    mod = _audit_module()

    def run(body):
        f = tmp_path / "k.s"
        f.write_text("_Z9my_kernelv:\n" + body + "\n.Lfunc_end0:\n")
        return mod.audit(str(f), "my_kernel")

    load = ";;#ASMSTART\nbuffer_load_dwordx4 v[4:7], v1, s[0:3], s4 offen\n;;#ASMEND\n"
    dma = "buffer_load_dwordx4 v1, s[0:3], 0 offen lds\n"
    assert run(load + dma + "s_waitcnt vmcnt(1)\nv_mfma_f32_16x16x32_f16 v[8:11], v[4:7], v[12:15], v[8:11]\ns_endpgm") == []
    assert any("touches" in p for p in run(load + dma + dma + "s_waitcnt vmcnt(3)\nv_add_f32 v9, v4, v4\ns_waitcnt vmcnt(0)\ns_endpgm"))
    assert any("touches" in p for p in run(load + "v_mov_b32 v5, 0\ns_waitcnt vmcnt(0)\ns_endpgm"))          # overwritten in flight
    assert any("s_endpgm" in p for p in run(load + "s_endpgm"))                                                   # never drained
    # a loop whose back edge skips the wait on one path
    loop = (".LBB0_1:\n" + load + "s_cbranch_scc1 .LBB0_2\ns_waitcnt vmcnt(0)\n.LBB0_2:\nv_add_f32 v9, v6, v6\n"
            "s_cbranch_vccnz .LBB0_1\ns_waitcnt vmcnt(0)\ns_endpgm")
    assert any("touches" in p for p in run(loop))
    good = (".LBB0_1:\n" + load + dma + "s_waitcnt vmcnt(1)\nv_add_f32 v9, v6, v6\ns_cbranch_vccnz .LBB0_1\ns_waitcnt vmcnt(0)\ns_endpgm")
    assert run(good) == []
