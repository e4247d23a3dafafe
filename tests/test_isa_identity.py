"""profiles/isa_identity.py's kernel-by-kernel comparison, on synthetic assembly texts of two tiny kernels (no compiler, no GPU).

A host-side change that names a template's instantiations in another order makes the compiler emit the same kernels in another order and renumber
their local labels: that has to come out as "same code".  A changed instruction, a changed descriptor field or a missing kernel must not."""
import importlib.util
import os

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_spec = importlib.util.spec_from_file_location("isa_identity", os.path.join(ROOT, "profiles", "isa_identity.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


def kernel(name, number, vgprs=8, add="v_add_f32_e32 v1, v0, v0", note="%bb.0"):
    """one kernel as the compiler writes it: the function with two local labels and a jump-table reference, then its descriptor block"""
    return f"""\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                ; @{name}
; {note}:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0

\tv_mov_b32_e32 v0, 0
\ts_cbranch_scc1 .LBB{number}_2
; %bb.1:                                ; {note}
\t{add}
\ts_getpc_b64 s[2:3]
\ts_add_u32 s2, s2, .LJTI{number}_0@rel32@lo+4
.LBB{number}_2:                         ; %Flow{number}
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v0, v1, s[0:1]
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{number}:
\t.size\t{name}, .Lfunc_end{number}-{name}
                                        ; -- End function
\t.set {name}.num_vgpr, {vgprs}
; Kernel info:
; NumVgprs: {vgprs}
"""


def unit(*kernels):
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.text\n" + "".join(kernels) + "\t.section\t\".note.GNU-stack\",\"\",@progbits\n").encode()


OLD = unit(kernel("_Z3k_aPf", 0), kernel("_Z3k_bPf", 1, vgprs=12, add="v_mul_f32_e32 v1, v0, v0"))


def test_kernel_code_takes_label_to_descriptor_without_comments_and_function_numbers():
    code = isa.kernel_code(OLD)
    assert sorted(code) == ["_Z3k_aPf", "_Z3k_bPf"]
    a = code["_Z3k_aPf"].decode().split("\n")
    assert a[0] == "_Z3k_aPf:" and a[-1].strip() == ".end_amdhsa_kernel"
    assert not any(";" in ln or not ln.strip() for ln in a)
    assert "\ts_cbranch_scc1 .LBB#_2" in a and ".LBB#_2:" in a and any(".LJTI#_0@rel32@lo+4" in ln for ln in a)
    assert any(ln.split() == [".amdhsa_next_free_vgpr", "8"] for ln in a)
    assert "v_mul_f32_e32 v1, v0, v0" in code["_Z3k_bPf"].decode() and "v_mul_f32" not in code["_Z3k_aPf"].decode()


def test_swapped_order_renumbered_labels_and_changed_comments_are_the_same_code():
    new = unit(kernel("_Z3k_bPf", 0, vgprs=12, add="v_mul_f32_e32 v1, v0, v0", note="%entry"), kernel("_Z3k_aPf", 7, note="%start"))
    assert new != OLD
    assert isa.same_code(OLD, new) == (True, [])
    assert isa.same_code(OLD, OLD) == (True, [])


def test_a_changed_instruction_differs():
    new = unit(kernel("_Z3k_aPf", 0), kernel("_Z3k_bPf", 1, vgprs=12, add="v_mul_f32_e32 v1, v0, v1"))
    same, why = isa.same_code(OLD, new)
    assert not same and len(why) == 1 and why[0].startswith("_Z3k_bPf:") and "v_mul_f32_e32 v1, v0, v1" in why[0]


def test_a_changed_register_count_differs():
    new = unit(kernel("_Z3k_aPf", 0, vgprs=9), kernel("_Z3k_bPf", 1, vgprs=12, add="v_mul_f32_e32 v1, v0, v0"))
    same, why = isa.same_code(OLD, new)
    assert not same and len(why) == 1 and why[0].startswith("_Z3k_aPf:") and ".amdhsa_next_free_vgpr 9" in why[0]


def test_a_missing_or_an_added_kernel_differs():
    only_a = unit(kernel("_Z3k_aPf", 0))
    assert isa.same_code(OLD, only_a) == (False, ["only in old: _Z3k_bPf"])
    assert isa.same_code(only_a, OLD) == (False, ["only in new: _Z3k_bPf"])
    # a label that merely moved to another block of the same function is a difference too: only the FUNCTION number is a placeholder
    moved = OLD.replace(b"s_cbranch_scc1 .LBB1_2", b"s_cbranch_scc1 .LBB1_3")
    assert moved != OLD and not isa.same_code(OLD, moved)[0]
