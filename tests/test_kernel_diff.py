"""tools/kernel_diff.py: the disassembly normaliser and the metadata comparison (CPU only).

The tool proves that a refactor left every gfx950 kernel as it was: per kernel symbol the register,
LDS, scratch and kernarg sizes of the metadata and a hash of the disassembly without the address
comments. The samples below are short literal texts in the formats of `llvm-objdump -d
--no-show-raw-insn` and `llvm-readelf --notes`; the last test runs the tool's own pipeline on the
built library against itself.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "i3dr_stereo_camera-ros_amd", "lib", "libsgm_hip.so")


def _tool():
    spec = importlib.util.spec_from_file_location("sgm_kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KD = _tool()

ASM_AT_1900 = """
Disassembly of section .text:

0000000000001900 <_ZN3sgm3k_aEPi>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                           // 000000001900: C0060002 00000000
\ts_cbranch_scc0 3                                            // 000000001908: BF840003 <_ZN3sgm3k_aEPi+0x18>
\tv_mov_b32_e32 v0, 0                                         // 00000000190C: 7E000280
\ts_endpgm                                                    // 000000001918: BF810000
\t\t...

0000000000001a00 <_ZN3sgm3k_bEPi>:
\ts_endpgm                                                    // 000000001A00: BF810000
"""

# the same kernels at other addresses (k_a without the padding that followed it)
ASM_AT_2500 = """
Disassembly of section .text:

0000000000002500 <_ZN3sgm3k_aEPi>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                           // 000000002500: C0060002 00000000
\ts_cbranch_scc0 3                                            // 000000002508: BF840003 <_ZN3sgm3k_aEPi+0x18>
\tv_mov_b32_e32 v0, 0                                         // 00000000250C: 7E000280
\ts_endpgm                                                    // 000000002518: BF810000

000000000000251c <_ZN3sgm3k_bEPi>:
\ts_endpgm                                                    // 00000000251C: BF810000
"""


def _notes(vgpr_a):
    return f"""
Displaying notes found in: .note
  Owner                Data size 	Description
  AMDGPU               0x00000400	NT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           out
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 512
    .kernarg_segment_align: 8
    .kernarg_segment_size: 8
    .max_flat_workgroup_size: 256
    .name:           _ZN3sgm3k_aEPi
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .symbol:         _ZN3sgm3k_aEPi.kd
    .vgpr_count:     {vgpr_a}
  - .agpr_count:     0
    .args:           []
    .group_segment_fixed_size: 0
    .kernarg_segment_align: 4
    .kernarg_segment_size: 0
    .max_flat_workgroup_size: 64
    .name:           _ZN3sgm3k_bEPi
    .private_segment_fixed_size: 0
    .sgpr_count:     4
    .symbol:         _ZN3sgm3k_bEPi.kd
    .vgpr_count:     1
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
"""


def _kernels(asm, notes):
    return KD.code_object_kernels(asm, notes)


def test_same_body_at_two_addresses_compares_equal():
    a, b = KD.kernel_bodies(ASM_AT_1900), KD.kernel_bodies(ASM_AT_2500)
    assert sorted(a) == sorted(b) == ["_ZN3sgm3k_aEPi", "_ZN3sgm3k_bEPi"]
    assert "s_cbranch_scc0 3" in KD.normalise(a["_ZN3sgm3k_aEPi"])          # the relative operand stays
    assert "1900" not in KD.normalise(a["_ZN3sgm3k_aEPi"])
    for k in a:
        assert KD.body_hash(a[k]) == KD.body_hash(b[k]), k
    assert KD.compare(_kernels(ASM_AT_1900, _notes(24)), _kernels(ASM_AT_2500, _notes(24))) == []


def test_one_changed_instruction_compares_different():
    changed = ASM_AT_2500.replace("v_mov_b32_e32 v0, 0 ", "v_mov_b32_e32 v1, 0 ")
    assert changed != ASM_AT_2500
    diffs = KD.compare(_kernels(ASM_AT_1900, _notes(24)), _kernels(changed, _notes(24)))
    assert [n for n, _ in diffs] == ["_ZN3sgm3k_aEPi"]
    assert len(diffs[0][1]) == 1 and diffs[0][1][0].startswith("body:")


def test_changed_vgpr_count_is_reported():
    md = KD.kernel_metadata(_notes(24))
    assert md["_ZN3sgm3k_aEPi"] == {".vgpr_count": "24", ".agpr_count": "0", ".sgpr_count": "12",
                                    ".group_segment_fixed_size": "512", ".private_segment_fixed_size": "0",
                                    ".kernarg_segment_size": "8", ".max_flat_workgroup_size": "256"}
    diffs = KD.compare(_kernels(ASM_AT_1900, _notes(24)), _kernels(ASM_AT_1900, _notes(32)))
    assert diffs == [("_ZN3sgm3k_aEPi", [".vgpr_count: 24 -> 32"])]


def test_missing_kernel_is_reported():
    old = _kernels(ASM_AT_1900, _notes(24))
    new = {k: v for k, v in old.items() if k != "_ZN3sgm3k_bEPi"}
    assert KD.compare(old, new) == [("_ZN3sgm3k_bEPi", ["only in OLD"])]
    assert KD.compare(new, old) == [("_ZN3sgm3k_bEPi", ["only in NEW"])]


def test_kernel_in_two_code_objects_is_an_error():
    lib = {}
    KD.merge_kernels(lib, _kernels(ASM_AT_1900, _notes(24)), "lib.so")
    assert sorted(lib) == ["_ZN3sgm3k_aEPi", "_ZN3sgm3k_bEPi"]
    with pytest.raises(RuntimeError, match="more than one code object: _ZN3sgm3k_aEPi, _ZN3sgm3k_bEPi"):
        KD.merge_kernels(lib, _kernels(ASM_AT_2500, _notes(24)), "lib.so")


def test_library_against_itself():
    if not os.path.exists(LIB):
        pytest.skip("libsgm_hip.so not built")
    for tool in ("clang-offload-bundler", "llvm-objdump", "llvm-readelf"):
        if not os.path.exists(os.path.join(KD.LLVM, tool)):
            pytest.skip(f"{tool} not available")
    ks = KD.library_kernels(LIB)
    assert len(ks) > 200, f"expected the library's kernels, found {len(ks)}"
    assert all(v["hash"] for v in ks.values()), "a kernel of the metadata has no disassembly"
    assert KD.compare(ks, KD.library_kernels(LIB)) == []
