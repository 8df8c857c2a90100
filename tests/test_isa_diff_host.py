"""tools/isa_diff.py, the per-function comparison of device assembly, on three short synthetic listings: the
function index in local labels and comments do not count, one changed instruction does, and a kernel may
move to a second file of its side."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def kernel(name, index, vgpr=8, op="v_add_f64 v[0:1], v[0:1], v[2:3]"):
    return """\t.text
\t.globl\t{n}
{n}:                                   ; @{n}
\ts_load_dword s0, s[4:5], 0x0       ; a trailing comment
; %bb.1:
\ts_cbranch_scc1 .LBB{i}_2
\t{op}
.LBB{i}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {n}
\t\t.amdhsa_next_free_vgpr {v}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{i}:
\t.size\t{n}, .Lfunc_end{i}-{n}
""".format(n=name, i=index, v=vgpr, op=op)


def device_fn(name, index):
    return "\t.text\n{n}:\n\tv_mov_b32 v0, 0\n\ts_setpc_b64 s[30:31]\n.Lfunc_end{i}:\n".format(n=name, i=index)


A = kernel("_Z3k_a", 0) + device_fn("_Z5g_ool", 1) + kernel("_Z3k_b", 2)


def test_equal_apart_from_label_numbering():
    b = kernel("_Z3k_b", 0) + kernel("_Z3k_a", 1) + device_fn("_Z5g_ool", 2)
    same, problems, ka, kb = isa_diff.compare([A], [b])
    assert (same, problems, ka, kb) == (3, [], 2, 2)


def test_one_changed_instruction_and_one_changed_descriptor():
    b = kernel("_Z3k_a", 0, op="v_fma_f64 v[0:1], v[0:1], v[2:3], v[0:1]") + device_fn("_Z5g_ool", 1) \
        + kernel("_Z3k_b", 2, vgpr=10)
    same, problems, _, _ = isa_diff.compare([A], [b])
    assert same == 1
    assert len(problems) == 2
    assert problems[0].startswith("differs (body;") and problems[0].endswith("_Z3k_a")
    assert problems[1].startswith("differs (descriptor;") and problems[1].endswith("_Z3k_b")


def test_kernel_moved_to_a_second_file(tmp_path):
    b1 = kernel("_Z3k_a", 0) + device_fn("_Z5g_ool", 1)
    b2 = device_fn("_Z5g_ool", 0) + kernel("_Z3k_b", 1)          # each file has its copy of the device function
    assert isa_diff.compare([A], [b1, b2]) == (3, [], 2, 2)
    # a kernel left behind is missing, one more is extra; copies that differ are reported
    same, problems, _, _ = isa_diff.compare([A], [b1, device_fn("_Z5g_ool", 0).replace("v0, 0", "v0, 1")
                                                  + kernel("_Z3k_c", 1)])
    assert same == 1
    assert problems == ["B: copies of _Z5g_ool differ between its files", "missing in B: _Z3k_b",
                        "extra in B: _Z3k_c", "differs (body; body 2 -> 2 lines): _Z5g_ool"]
    # the command line: exit status 0 / 1
    paths = []
    for name, text in (("a.s", A), ("b1.s", b1), ("b2.s", b2), ("c.s", kernel("_Z3k_a", 0))):
        (tmp_path / name).write_text(text)
        paths.append(str(tmp_path / name))
    assert isa_diff.main([paths[0], "--", paths[1], paths[2]]) == 0
    assert isa_diff.main([paths[0], "--", paths[3]]) == 1
