"""tools/isa_diff.py on two small hand-written listings: a kernel is its whole function, not the text up to its first s_endpgm.

No GPU and no compiler: the listings below have the shape of `hipcc -S --cuda-device-only` output -- a label per kernel, local labels,
directives, comments, a .Lfunc_end<n> label behind the last instruction and a kernel descriptor with the resource figures."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import isa_diff  # noqa: E402


def descriptor(name, vgpr):
    return f"""\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 1024
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t\t.amdhsa_accum_offset 8
\t.end_amdhsa_kernel
"""


# k_early leaves at once for the blocks of the other form (s_endpgm in front of its body), as k_ibp_dtile and k_ibp_sh do
EARLY_BODY = """\tv_mul_f32_e32 v2, v0, v1
\tv_add_f32_e32 v3, v2, v0
\tds_write_b32 v4, v3
"""
PLAIN_BODY = """\tv_mov_b32_e32 v1, 0
\tv_add_f32_e32 v2, v0, v1
\tglobal_store_dword v[4:5], v2, off
"""


def listing(early_body=EARLY_BODY, plain_body=PLAIN_BODY, plain_vgpr=6):
    return f"""\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.globl\tk_early
\t.p2align\t8
\t.type\tk_early,@function
k_early:                                ; @k_early
; %bb.0:
\ts_load_dword s4, s[0:1], 0x0
\ts_waitcnt lgkmcnt(0)
\ts_cmp_lg_u32 s4, 0
\ts_cbranch_scc1 .LBB0_2
; %bb.1:
\ts_endpgm
.LBB0_2:
{early_body}\ts_endpgm
\t.section\t.rodata,"a",@progbits
.Lfunc_end0:
\t.size\tk_early, .Lfunc_end0-k_early
{descriptor("k_early", 8)}\t.text
\t.globl\tk_plain
\t.type\tk_plain,@function
k_plain:                                ; @k_plain
; %bb.0:
{plain_body}\ts_endpgm
.Lfunc_end1:
\t.size\tk_plain, .Lfunc_end1-k_plain
{descriptor("k_plain", plain_vgpr)}"""


def run(tmp_path, capsys, old, new):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old)
    b.write_text(new)
    status = isa_diff.main([str(a), str(b), "-v"])
    return status, capsys.readouterr().out


def verdict_of(out, kernel):
    lines = [ln for ln in out.splitlines()[1:] if f" {kernel}:" in ln]
    return lines[0].split()[0] if lines else "identical"


def test_kernel_text_runs_to_its_function_end():
    ks = isa_diff.kernels(listing())
    assert list(ks) == ["k_early", "k_plain"]
    early, figs = ks["k_early"]
    assert [ln.split()[0] for ln in early].count("s_endpgm") == 2 and early[-2].startswith("ds_write_b32")
    assert figs == {"group_segment_fixed_size": "1024", "private_segment_fixed_size": "0", "next_free_vgpr": "8", "next_free_sgpr": "16", "accum_offset": "8"}
    assert ks["k_plain"][0][0].startswith("v_mov_b32") and len(ks["k_plain"][0]) == 4  # nothing of the directives behind k_early's end


def test_change_behind_the_first_endpgm_is_changed(tmp_path, capsys):
    status, out = run(tmp_path, capsys, listing(), listing(early_body=EARLY_BODY.replace("v_add_f32_e32 v3, v2, v0", "v_sub_f32_e32 v3, v2, v0")))
    assert status == 1
    assert verdict_of(out, "k_early") == "CHANGED" and verdict_of(out, "k_plain") == "identical"
    assert "1 identical" in out and "1 CHANGED" in out


def test_register_renumbering_is_renamed(tmp_path, capsys):
    status, out = run(tmp_path, capsys, listing(), listing(early_body=EARLY_BODY.replace("v2", "v7").replace("v3", "v6")))
    assert status == 0
    assert verdict_of(out, "k_early") == "renamed" and "1 renamed" in out and "0 CHANGED" in out


def test_swap_of_two_instructions_is_reordered(tmp_path, capsys):
    swapped = "".join(PLAIN_BODY.splitlines(keepends=True)[i] for i in (1, 0, 2))
    status, out = run(tmp_path, capsys, listing(), listing(plain_body=swapped))
    assert status == 0
    assert verdict_of(out, "k_plain") == "reordered" and verdict_of(out, "k_early") == "identical" and "1 reordered" in out


def test_differing_vgpr_figure_fails(tmp_path, capsys):
    status, out = run(tmp_path, capsys, listing(), listing(plain_vgpr=7))
    assert status == 1
    assert "FIGURES next_free_vgpr 6->7" in out and verdict_of(out, "k_plain") == "identical" and "2 identical" in out


def test_listing_against_itself_is_identical(tmp_path, capsys):
    status, out = run(tmp_path, capsys, listing(), listing())
    assert status == 0
    assert "2 identical, 0 renamed, 0 reordered, 0 CHANGED" in out and len(out.strip().splitlines()) == 1
