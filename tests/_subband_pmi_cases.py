"""The (case of tests/test_gpu_codebook_rate.py, subband size) pairs of the subband-PMI tests, shared by
tests/test_subband_pmi_cpu.py (the conditions on the inputs) and tests/test_gpu_subband_pmi.py.  The shapes are the smallest at
which each part of the subband nest of k10_codebook_rate.hip can go wrong; a plain module, no torch, no GPU."""

from tests._consumer_shapes import SUBBAND_CASES as _EVERY_PAIR

SUBBAND_CASES = [
    # one subband: all six outputs are dmx_codebook_rate's, bit for bit
    ("K65", 65), ("K65", 1000),
    # subband = chunk edge; K65: a last subband of one subcarrier
    ("K63", 64), ("K64", 64), ("K65", 64),
    ("K65", 16),                                     # 5 subbands, kcp = 16, the last of 1
    ("slices_K7", 1), ("slices_K7", 3),              # kcp = 1 (64 slices); kcp = 4 with a short last subband
    ("slices_K33", 4), ("slices_K33", 32),           # 9 subbands at L = 2; a last subband of 1 under kcp = 32
    ("K512", 100), ("K512", 128), ("K512", 4),       # subbands of 64 + 36; two full chunks; 128 subbands (more than a wave's lanes)
    # one and two row chunks: the running best of a subband across row chunks
    ("L1_C32", 1), ("L1_C32", 2), ("L1_C33", 1), ("L1_C33", 2),
    # whole-codeword chunk edges at L = 3, 4
    ("L3_C11", 1), ("L3_C11", 2), ("L4_C8", 1), ("L4_C8", 2), ("L4_C9", 1), ("L4_C9", 2),
    ("panel_C64", 4),                                # 256-element panel, two row chunks, 4 subbands
    ("C1", 2), ("L2_4x2", 2), ("defaults", 1),       # fewer codewords than slices; K = 1
    ("irregular", 4),                                # int32-extreme subcarrier indices inside subbands
    # users without a path (+0.0 / -1 everywhere), rank-one users
    ("counts_and_holes", 2), ("one_path", 2), ("rot_fov_dipole", 2),
    # launch residue at 4 and 2 waves per workgroup
    ("wpb4_users41", 1), ("wpb4_users41", 16), ("wpb4_users42", 1), ("wpb4_users42", 16),
    ("wpb4_users43", 1), ("wpb4_users43", 16), ("wpb2_users7", 1), ("wpb2_users7", 16),
    # stage-1 features through the records
    ("per_user_rot", 1), ("doppler", 2), ("adaptive_workspace", 5),
]
# every (M_rx, layers) pair at K = 3 under subbands of 2: a full subband and a short last one
SUBBAND_CASES += _EVERY_PAIR

# compute_csi_report: the cases whose references pick at least two ranks (tests/test_subband_pmi_cpu.py holds that), ranks 1..4
RANK_CASES = ("slices_K7", "L4_4x4")
RANK_LAYERS = (1, 2, 3, 4)
RANK_CODEWORDS = 16
RANK_SUBBANDS = (3, None)


def case_label(cid, B):
    return f"{cid}-B{B}"
