"""Numpy / Python model of the reference's probability passes over a frame's RECORDS (what k_token_counts and k_token_probs compute):
accumulate_token_branches (serializer.cc:456-586) -> branch counts [4][8][3][11][2] {false, true}, Encoder::calc_prob (encoder.cc:48-55),
optimize_probability_tables (encoder.cc:419-439), optimize_prob_skip (:442-457), optimize_interframe_probs (encode_inter.cc:525-575).
Written from the reference's text, independently of serialize_common.hh."""
import numpy as np

import rebase_model as rm

ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
BAND = [0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7]
Y_AFTER_Y2, Y2, UV, Y_WITHOUT_Y2 = 0, 1, 2, 3
SKIP, HAS_Y2 = 8, 2


def count_block(counts, kind, coefficients, context):
    """One block: `coefficients` in zigzag order."""
    first = 1 if kind == Y_AFTER_Y2 else 0
    coded = 0
    for i in range(first, 16):
        if coefficients[i]:
            coded = i + 1
    last_was_zero, ctx, i = False, context, first
    while i < coded:
        c = counts[kind, BAND[i], ctx]
        v = abs(int(coefficients[i]))
        if not last_was_zero:
            c[0, 1] += 1
        i += 1
        if v == 0:
            c[1, 0] += 1; last_was_zero = True; ctx = 0
            continue
        last_was_zero = False
        c[1, 1] += 1
        if v == 1:
            c[2, 0] += 1; ctx = 1
            continue
        ctx = 2
        c[2, 1] += 1
        if v == 2:
            c[3, 0] += 1; c[4, 0] += 1
        elif v == 3:
            c[3, 0] += 1; c[4, 1] += 1; c[5, 0] += 1
        elif v == 4:
            c[3, 0] += 1; c[4, 1] += 1; c[5, 1] += 1
        else:
            c[3, 1] += 1
            if v < 7:
                c[6, 0] += 1; c[7, 0] += 1
            elif v < 11:
                c[6, 0] += 1; c[7, 1] += 1
            else:
                c[6, 1] += 1
                if v < 19:
                    c[8, 0] += 1; c[9, 0] += 1
                elif v < 35:
                    c[8, 0] += 1; c[9, 1] += 1
                else:
                    c[8, 1] += 1
                    c[10, 0 if v < 67 else 1] += 1
    if coded < 16:
        counts[kind, BAND[i], ctx][0, 0] += 1


def mask(rec):
    return 0 if rec["flags"] & SKIP else int(rec["nz_mask"])


def branch_counts(mb, blocks):
    """Every macroblock's Y, U and V blocks (Y2 blocks are not counted; macroblocks whose tokens are skipped are) -> uint32 [4, 8, 3, 11, 2]."""
    dense = rm.dense(mb, blocks)
    mbh, mbw = mb.shape
    counts = np.zeros((4, 8, 3, 11, 2), np.uint32)
    for r in range(mbh):
        for c in range(mbw):
            nz = mask(mb[r, c])
            above = mask(mb[r - 1, c]) if r else 0
            left = mask(mb[r, c - 1]) if c else 0
            y2 = bool(mb[r, c]["flags"] & HAS_Y2)
            for b in range(24):
                if b < 16:
                    a = (nz >> (b - 4)) & 1 if b >= 4 else (above >> (12 + b)) & 1
                    l = (nz >> (b - 1)) & 1 if b & 3 else (left >> (b + 3)) & 1
                    kind = Y_AFTER_Y2 if y2 else Y_WITHOUT_Y2
                else:
                    k = (b - 16) & 3
                    a = (nz >> (b - 2)) & 1 if k >= 2 else (above >> (b + 2)) & 1
                    l = (nz >> (b - 1)) & 1 if k & 1 else (left >> (b + 1)) & 1
                    kind = UV
                coeffs = dense[r, c, b][ZIGZAG] if (nz >> b) & 1 else np.zeros(16, np.int16)
                count_block(counts, kind, coeffs, a + l)
    return counts


def calc_prob(false_count, total):
    return 0 if false_count == 0 else max(1, min(255, 256 * int(false_count) // int(total)))


def token_updates(counts, before):
    """optimize_probability_tables -> (update flags [1056], values [1056] (0 where no update), the frame's table [1056])."""
    c = counts.reshape(1056, 2)
    before = np.asarray(before, np.uint8).reshape(-1)[:1056]
    prob = np.array([calc_prob(f, int(f) + int(t)) for f, t in c], np.int32)
    update = (prob > 0) & (prob != before)
    return update, np.where(update, prob, 0).astype(np.uint8), np.where(update, prob, before).astype(np.uint8)


def frame_probs(mb):
    """optimize_prob_skip, optimize_interframe_probs -> (prob_skip_false, prob_inter, prob_references_last, prob_references_golden); 0 = not set."""
    n = mb.size
    has = int(((mb["nz_mask"] != 0) & ((mb["flags"] & SKIP) == 0)).sum())
    r = [int((mb["ref_frame"] == k).sum()) for k in range(4)]
    return calc_prob(has, n), calc_prob(r[0], sum(r)), calc_prob(r[1], r[1] + r[2] + r[3]), calc_prob(r[2], r[2] + r[3])
