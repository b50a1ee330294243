"""tools/isa_issue.py on a small hand-written assembly: the kernel is found by its name, a
net body is the innermost loop with product MFMAs, every instruction lands in one class
and the two cycle sums follow the price list (MFMA 8 of issue and 16 / 8 of pipe, plain
VALU 4, conversion 4.5, transcendental 8)."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_issue as T  # noqa: E402

NAME = "_ZN2df14uniform_kernelILi4ELi0ELb1ELb1ELb1ELb1EEEvNS_9ChainArgsE"
OTHER = "_ZN2df14uniform_kernelILi4ELi0ELb1ELb1ELb0ELb0EEEvNS_9ChainArgsE"
BODY = """\
.LBB0_2:                                ; the net body
\tds_read_b128 v[0:3], v40
\tds_read_b32 v4, v41 offset:16
\ts_waitcnt lgkmcnt(0)
\tv_cvt_pk_bf16_f32 v5, v4, v4
\tv_lshlrev_b32_e32 v6, 16, v5
\tv_sub_f32 v7, v4, v6
\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[8:11], 0
\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[8:11], a[0:3]
\tv_mfma_f32_4x4x4_16b_bf16 a[4:7], v[12:13], v[14:15], a[4:7]
\ts_nop 3
\tv_accvgpr_read_b32 v16, a0
\tv_max_i32_e32 v16, 0, v16
\tv_exp_f32_e32 v17, v16
\tv_nop
\ts_nop 0
\tv_permlane16_swap_b32_e32 v17, v16
\tds_write_b32 v41, v17
\ts_add_i32 s4, s4, 1                    ; v_fake_in_comment ds_read_b32
\ts_cmp_lt_i32 s4, s5
\ts_cbranch_scc1 .LBB0_2
"""


def _asm():
    head = f"\t.globl\t{NAME}\n{NAME}:\n\ts_mov_b32 s4, 0\n.LBB0_1:                                ; the layer loop\n\tv_mov_b32_e32 v40, 0\n"
    tail = ("\ts_cbranch_scc0 .LBB0_1\n\ts_endpgm\n.Lfunc_end0:\n"
            "; NumVgprs: 42\n; ScratchSize: 0\n; Occupancy: 4\n")
    other = (f"{OTHER}:\n.LBB1_1:\n\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[8:11], 0\n\tv_mov_b32_e32 v1, v2\n"
             "\ts_cbranch_scc1 .LBB1_1\n\ts_endpgm\n.Lfunc_end1:\n; NumVgprs: 9\n; ScratchSize: 16\n; Occupancy: 8\n")
    pad = "; metadata\n" * 64  # isa_waits.stats reads the 60 lines behind a kernel
    return (head + BODY + tail + pad + other).splitlines()


def test_classes():
    for op, want in (("v_mfma_f32_16x16x32_bf16", "mfma"), ("v_mfma_f32_4x4x4_16b_bf16", "mfma2"),
                     ("v_cvt_pk_bf16_f32", "cvt"), ("v_exp_f32_e32", "trans"), ("v_rcp_f32_e32", "trans"),
                     ("v_fmac_f32_e32", "valu"), ("v_cndmask_b32_e32", "valu"), ("v_cvt_f32_i32_e32", "valu"),
                     ("v_nop", None), ("ds_read2_b32", "ds_read"), ("ds_write_b64", "ds_write"),
                     ("s_nop", "s_nop"), ("s_waitcnt", "s_waitcnt"), ("s_and_saveexec_b64", None),
                     ("s_cbranch_scc1", None), ("global_load_lds_dwordx4", None)):
        assert T.classify(op) == want, op


def test_body_census():
    lines = _asm()
    (name, a, b), _ = T.W.kernels(lines)
    assert name == NAME
    (la, lb), = T.W.bodies(lines, a, b)
    n, states = T.census(lines, la, lb)
    assert n == {"mfma": 2, "mfma2": 1, "valu": 5, "cvt": 1, "trans": 1, "ds_read": 2, "ds_write": 1, "s_nop": 2,
                 "s_waitcnt": 1}
    assert states == 4 + 1
    assert T.issue_cycles(n) == 8 * 3 + 4 * 5 + 4.5 + 8
    assert T.pipe_cycles(n) == 16 * 2 + 8


def test_report_selects_kernels():
    out = io.StringIO()
    assert T.report(_asm(), T.DEFAULT, out) == 1
    text = out.getvalue().splitlines()
    assert text[0] == f"{NAME}: VGPRs 42 scratch 0 occupancy 4"
    assert "mfma 2 mfma2 1 valu 5 cvt 1 trans 1 ds_r 2 ds_w 1 nop 2 [5] wait 1 issue 56 pipe 40" in text[1]
    assert text[2].startswith("  mean of 1 bodies: valu+cvt+trans 7.0 ")
    out = io.StringIO()
    assert T.report(_asm(), "uniform_kernel", out) == 2
    assert "scratch 16 occupancy 8" in out.getvalue()
    assert T.report(_asm(), "no_such_kernel", io.StringIO()) == 0
