"""The gradient-tile table of the one-launch training kernel (vjf_mega_grad_tiles, vjf_amd/csrc/vjf_mega_common.h; export
vjf_mega_grad_tile_table), checked on the CPU against a restatement of the late slab's layout (vjf_mega_slab_layout) and of the trial
role's LDS layout (vjf_mega_trial_lds) for a sweep of plans: every stored float of the slab is covered by exactly one tile, no tile
reaches outside its block, every tile's operand rows are the tensor's, and the eight wavefronts' shares differ by at most one tile."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

from vjf_amd import _native as N

HDR, ENT, NW, LD, TR, RS_N = 16, 8, 8, 33, 32, 8


def table(dy, dz, du, hidden, n=32):
    cfg = N.make_config(dy, dz, du, n, hidden, N.LIK_GAUSSIAN, 64)
    L = N.lib()
    words = C.c_int32()
    assert L.vjf_mega_grad_tile_table(C.byref(cfg), None, 0, C.byref(words)) == 0
    buf = (C.c_int32 * words.value)()
    assert L.vjf_mega_grad_tile_table(C.byref(cfg), buf, words.value, None) == 0
    return np.array(buf, dtype=np.int64)


def slab_blocks(dy, dz, du, hidden):
    """(offset, ldm, rows, M, Kin) per block, in the slab's order: decoder, mean head (no bias), log-variance head, layers L-1 .. 0."""
    din, hL = dy + du + 2 * dz, hidden[-1]
    shapes = [(dy, dz, dz + 1), (dz, hL, hL), (dz, hL, hL + 1)]
    for l in range(len(hidden) - 1, -1, -1):
        kin = hidden[l - 1] if l > 0 else din
        shapes.append((hidden[l], kin, kin + 1))
    out, o = [], 0
    for M, kin, rows in shapes:
        ldm = (M + 3) & ~3
        out.append((o, ldm, rows, M, kin))
        o += rows * ldm
    return out, o


def lds_layout(dy, dz, du, hidden, n):
    """First float of the LDS matrices the gradient tiles read (the order of vjf_mega_trial_lds; every region padded to 4 floats)."""
    din, dxu, hmax, hsum, nl = dy + du + 2 * dz, dz + du, max(hidden), sum(hidden), len(hidden)
    o, at = 0, {}

    def take(name, nfl):
        nonlocal o
        at[name] = o
        o += (nfl + 3) & ~3
    npad = (n + 3) & ~3
    take("cen", npad * dxu); take("iw", npad)
    take("in", din * LD); take("xu", dxu * LD); take("phi", n * LD); take("act", hsum * LD)
    compact = dy >= hmax
    nd = (1 if nl > 1 else 0) if compact else (2 if nl > 1 else 1)
    take("dd", nd * hmax * LD)
    for name in ("mu", "lv", "xt", "e2", "pm", "dmu", "dlv", "dx"):
        take(name, dz * LD)
    take("xn", dxu * LD); take("py", dy * LD); take("dpy", dy * LD)
    at["d0"] = at["py"] if compact else at["dd"]
    at["d1"] = at["dd"] if compact else at["dd"] + hmax * LD
    return at


def check_plan(dy, dz, du, hidden, n=32):
    t = table(dy, dz, du, hidden, n)
    nt, nseg = int(t[0]), int(t[1])
    nl = len(hidden)
    assert len(t) == HDR + ENT * nt
    ends = [int(x) for x in t[2:2 + nseg]]
    assert nseg == 1 + max(0, nl - 2) and ends == sorted(ends) and ends[-1] == nt
    blocks, slab_len = slab_blocks(dy, dz, du, hidden)
    at = lds_layout(dy, dz, du, hidden, n)
    din, hsum = dy + du + 2 * dz, sum(hidden)
    # operand bases per block: (first float of D, first float of Bact)
    hact = at["act"] + (hsum - hidden[-1]) * LD
    bases = [(at["dpy"], at["xt"]), (at["dmu"], hact), (at["dlv"], hact)]
    for l in range(nl - 1, -1, -1):
        d = at["d1"] if (nl - 1 - l) & 1 else at["d0"]
        bases.append((d, at["act"] + sum(hidden[:l - 1]) * LD if l > 0 else at["in"]))
    cover = np.zeros(slab_len, dtype=np.int32)
    blk_of_tile = []
    for q in range(nt):
        a_off, mval, b_off, kval, s_off, ldm, jval, mlim = (int(x) for x in t[HDR + ENT * q:HDR + ENT * (q + 1)])
        b = max(k for k, blk in enumerate(blocks) if blk[0] <= s_off)
        off, bl_ldm, rows, M, kin = blocks[b]
        blk_of_tile.append(b)
        j0, m0 = divmod(s_off - off, bl_ldm)
        assert ldm == bl_ldm and j0 % 16 == 0 and m0 % 16 == 0 and j0 < rows and m0 < ldm
        assert jval == rows - j0 and mlim == ldm - m0 and mval == M - m0 and kval == kin - j0
        assert mval > 0 and kval >= 0
        assert a_off == bases[b][0] + m0 * LD and b_off == bases[b][1] + j0 * LD
        # what the 64 lanes store: lane (i, kk) the four floats of row j0 + i at column m0 + 4 kk, if i < jval and 4 kk < mlim
        for i in range(min(16, jval)):
            for kk in range(4):
                if 4 * kk < mlim:
                    lo = s_off + i * ldm + 4 * kk
                    assert off <= lo and lo + 4 <= off + rows * ldm, "a tile stores outside its block"
                    cover[lo:lo + 4] += 1
    assert (cover == 1).all(), "every float of the late slab is stored by exactly one tile"
    # segments: 0 = decoder, heads, the last two layers; then one per deeper layer
    for q, b in enumerate(blk_of_tile):
        seg = next(s for s, e in enumerate(ends) if q < e)
        assert (b <= 4 and seg == 0) or (b >= 5 and seg == b - 4)
    assert blk_of_tile == sorted(blk_of_tile)
    # the walk: wavefront w takes w, w + 8, ... segment by segment
    share, seen = [0] * NW, np.zeros(nt, dtype=np.int32)
    for w in range(NW):
        q = w
        for e in ends:
            while q < e:
                seen[q] += 1
                share[w] += 1
                q += NW
    assert (seen == 1).all() and max(share) - min(share) <= 1
    return nt


WIDTHS = [1, 3, 4, 5, 15, 16, 17, 20, 31, 32, 33, 48]


@pytest.mark.parametrize("nl", list(range(1, N.MAX_HIDDEN + 1)))
def test_table_covers_the_slab(nl):
    rng = random.Random(100 + nl)
    for dz in range(1, 17):
        for dy, du in ((16, 0), (17, 2), (50, 0)):
            hidden = [rng.choice(WIDTHS) for _ in range(nl)]
            check_plan(dy, dz, du, hidden)


def test_every_width_pair_at_two_layers():
    for h0, h1 in itertools.product(WIDTHS, WIDTHS):
        check_plan(17, 3, 0, [h0, h1])


def test_config_b_drops_the_mean_heads_bias_tile():
    # decoder 4 x 1, mean head 1 x 9 of which the ninth holds only the ones row (no bias: nothing to store), log-variance head 1 x 9,
    # layer 0: 8 x 5
    assert check_plan(50, 10, 0, [128], n=200) == 4 + 8 + 9 + 40
    # hL + 1 = 16: the bias is the last column of a full tile -- nothing to drop but the mean head's tile has 15 rows to store
    assert check_plan(17, 3, 0, [15]) == 2 * 1 + 1 + 1 + 1 * 2
    assert check_plan(17, 3, 0, [16]) == 2 * 1 + 1 + 2 + 1 * 2


def test_capacity_is_checked():
    cfg = N.make_config(17, 3, 0, 32, [16], N.LIK_GAUSSIAN, 64)
    buf = (C.c_int32 * 8)()
    assert N.lib().vjf_mega_grad_tile_table(C.byref(cfg), buf, 8, None) == -7
    assert b"vjf_mega_grad_tile_table" in N.lib().vjf_last_error()
