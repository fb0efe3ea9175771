"""A host model of how conv_hxi's split forms enumerate their output pixels (pc_conv_hxi.hip):
which halo slot every (fragment, lane, tap) reads, and the LDS bank conflicts of those ds_read_b128.

14x14x256: the dense enumeration over the pitch-16 halo (HxiGeom DENSE, hxi_dense_pixel) - 196 pixels in 13
fragments: columns 0-7 of two rows in each of fragments 0-6, columns 8-13 of two rows and a pair of the pixels
left over in each of fragments 7-12. 28x28x128: 7 rows at pitch 29 (a row's right padding column is the next
row's left one), 203 slots in 13 fragments of consecutive slots, 7 + 6 over the two fragment wave groups.

LDS model (MI355X: 64 banks of 4 bytes; a wave's ds_read_b128 is served in four groups of 16 lanes, only the
lanes of a group conflict, equal addresses broadcast): a halo slot is 256 bytes = 16 chunks of 16 bytes, all
64 banks; chunk position p of slot h holds source chunk p ^ ((h & 7) << 1). Lane kg * 16 + fr reads chunk
blk * 4 + kg (hi) or 8 + blk * 4 + kg (lo) of its slot. The conflict degree of a read is the largest number of
distinct slots that one lane group asks for at one chunk position.

Asserted bounds: the pitch enumerations (16 consecutive slots per fragment) are conflict-free; the dense 14x14
one is conflict-free in fragments 0-6 and has degree 2 on the reads of fragments 7-12, and no enumeration of
the 196 pixels in 13 fragments avoids conflicts under this swizzle (a counting argument, below). The plain
enumeration q = 16 f + fr (measured and dropped) has degree 2 in 12 fragments."""
import itertools

# ds_read_b128's lane groups
GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]
TAPS = list(itertools.product(range(3), range(3)))


def dense_pixel(f, fr):
    """hxi_dense_pixel: (row, col) of fragment f's lane slot fr; col 14: a discarded lane."""
    if f < 7:
        return 2 * f + (fr >> 3), fr & 7
    j, c = f - 7, fr & 7
    if c < 6:
        return 2 * j + (fr >> 3), 8 + c
    if fr < 8:
        return 12 + j // 3, 8 + 2 * (j % 3) + (fr & 1)
    return 0, 14


def dense_slot(f, fr, pitch=16):
    """The kernel's arithmetic (conv_hxi_layer, the DENSE read group): (slot at tap (0, 0), the part of it in
    the read's immediate). The immediate part is a multiple of 8: it leaves the swizzle key to the lane's part."""
    imm = 32 * f if f < 7 else 32 * (f - 7) + 8
    lane = fr + (fr & 8)
    if f >= 7 and (fr & 14) == 6:
        j = f - 7
        lane = (fr & 1) + (12 + j // 3) * pitch + 8 + 2 * (j % 3) - imm
    assert imm % 8 == 0 and 0 <= lane < 256
    return imm + lane, imm


def plain_dense_slot(HW, PITCH, NPIX, f, fr):
    """The plain dense enumeration (measured and dropped): pixel q = 16 f + fr at slot q + (PITCH - HW) (q / HW),
    the lanes past the last pixel on the last pixel's slot."""
    q = min(16 * f + fr, NPIX - 1)
    return q + (PITCH - HW) * (q // HW)


def degree(slots, blk, lo):
    """Conflict degree of one ds_read_b128: slots[fr] is the halo slot of lane slot fr (every kg reads it)."""
    worst = 0
    for grp in GROUPS:
        asked = {}
        for lane in grp:
            fr, kg = lane & 15, lane >> 4
            h = slots[fr]
            pos = (blk * 4 + kg + (8 if lo else 0)) ^ ((h & 7) << 1)
            asked.setdefault(pos, set()).add(h)
        assert sum(len(v) for v in asked.values()) <= 16
        worst = max(worst, max(len(v) for v in asked.values()))
    return worst


def read_degrees(frag_slots, pitch):
    """{(fragment, tap, block, lo): degree} over every read of the K loop."""
    out = {}
    for f, slots in enumerate(frag_slots):
        for (dy, dx), blk, lo in itertools.product(TAPS, range(2), range(2)):
            out[f, dy, dx, blk, lo] = degree([h + dy * pitch + dx for h in slots], blk, lo)
    return out


def staged_pixel(h, pitch, hw, rows):
    """Input pixel (row relative to the workgroup's first output row, column) that halo slot h holds, or None
    for a zero slot (the stage lambda of conv_hxi_layer)."""
    iy, ix = h // pitch - 1, h % pitch - 1
    return (iy, ix) if h < (rows + 2) * pitch and 0 <= ix < hw else None


# ---- 14x14x256, dense -------------------------------------------------------------------------------------
HW14, P14, NPIX14, NF14 = 14, 16, 196, 13
SLOTS14 = (HW14 - 1) * P14 + (HW14 - 1) + 2 * P14 + 2 + 1      # HxiGeom::SLOTS, DENSE


def frag14(f):
    return [dense_slot(f, fr)[0] for fr in range(16)]


def test_dense14_covers_every_pixel_once():
    assert SLOTS14 == 256 and (NPIX14 + 15) // 16 == NF14
    seen = {}
    for f in range(NF14):
        for fr in range(16):
            r, c = dense_pixel(f, fr)
            h, _ = dense_slot(f, fr)
            if c < HW14:
                assert 0 <= r < HW14 and h == r * P14 + c            # the pixel's halo slot at tap (0, 0)
                assert (r, c) not in seen
                seen[r, c] = h
    assert sorted(seen) == [(r, c) for r in range(HW14) for c in range(HW14)]
    # every tap of a real pixel reads the input pixel it should, or a zero slot outside the map
    for (r, c), h in seen.items():
        for dy, dx in TAPS:
            want = (r - 1 + dy, c - 1 + dx)
            got = staged_pixel(h + dy * P14 + dx, P14, HW14, HW14)
            assert got == (want if 0 <= want[1] < HW14 else None), (r, c, dy, dx)


def test_dense14_reads_stay_in_the_stage():
    discarded, top = 0, 0
    for f in range(NF14):
        for fr in range(16):
            h, _ = dense_slot(f, fr)
            real = dense_pixel(f, fr)[1] < HW14
            discarded += not real
            for dy, dx in TAPS:
                assert 0 <= h + dy * P14 + dx < SLOTS14, (f, fr, dy, dx)
            if real:
                top = max(top, h)
            else:     # lanes 14 and 15 of fragments 7-12: the padding columns of the fragment's second row
                assert f >= 7 and fr >= 14 and h == (2 * (f - 7) + 1) * P14 + fr
    assert discarded == 16 * NF14 - NPIX14 == 12
    # the last pixel's last tap is the stage's last slot: nothing is staged for the discarded lanes alone
    assert top + 2 * P14 + 2 == SLOTS14 - 1


def test_pitch_enumerations_are_conflict_free():
    """16 consecutive slots at any alignment: the 14x14 and 28x28 pitch forms, the 7x7 form (pitch 9), and the
    28x28 form at pitch 29."""
    for pitch, nf in ((16, 14), (32, 14), (9, 4), (29, 13)):
        deg = read_degrees([[16 * f + fr for fr in range(16)] for f in range(nf)], pitch)
        assert len(deg) == nf * 9 * 2 * 2 and set(deg.values()) == {1}, pitch


def test_dense14_conflict_degree():
    """Fragments 0-6: the 8 slots of a lane group's half are 4 + 4 of two rows with 8 different keys. Fragments
    7-12: lanes 6 and 7 hold pixels of columns 8-13, whose keys two other lanes of their half have: degree 2
    on every read of these 6 fragments (216 of the 13 x 9 x 2 x 2)."""
    deg = read_degrees([frag14(f) for f in range(NF14)], P14)
    assert len(deg) == NF14 * 9 * 2 * 2
    assert max(deg.values()) == 2
    assert {k[0] for k, v in deg.items() if v > 1} == set(range(7, NF14))
    assert sum(1 for v in deg.values() if v > 1) == 6 * 9 * 2 * 2


def test_plain_dense14_conflict_degree():
    """q = 16 f + fr: every full fragment meets a row boundary, its slots are two runs around a gap of 2, and two
    of the 8 slots of a half share their keys: degree 2 on every read of fragments 0-11."""
    frags = [[plain_dense_slot(HW14, P14, NPIX14, f, fr) for fr in range(16)] for f in range(NF14)]
    deg = read_degrees(frags, P14)
    assert max(deg.values()) == 2
    assert {k[0] for k, v in deg.items() if v > 1} == set(range(NF14 - 1))


def test_no_conflict_free_cover_in_13_fragments():
    """Under the swizzle a lane group is conflict-free iff each of its two 8-lane halves (one kg each) reads 8
    slots with 8 different keys h & 7. At pitch 16 the key is the pixel's column + a constant, mod 8: columns
    0-5 share their keys with columns 8-13, columns 6 and 7 have keys of their own, 14 pixels each. 13
    fragments are 26 halves, each with one pixel per key at most: room for 6 x 26 + 2 x 14 = 184 < 196."""
    per_key = [0] * 8
    for q in range(NPIX14):
        per_key[(q % HW14 + 1) & 7] += 1
    halves = 2 * NF14
    assert sum(min(n, halves) for n in per_key) == 184 < NPIX14


# ---- 28x28x128, 7 rows at pitch 29 ------------------------------------------------------------------------
HW28, P28, ROWS28, NF28, WPX28 = 28, 29, 7, 13, 2
TP28 = (NF28 + WPX28 - 1) // WPX28
SLOTS28 = (NF28 * 16 - ROWS28 * P28) + (ROWS28 + 2) * P28 + 2             # HxiGeom::SLOTS


def test_pitch29_covers_every_pixel_once():
    assert (ROWS28 * P28 + 15) // 16 == NF28 and TP28 == 7 and SLOTS28 == 268
    # the fragments of the two wave groups: wpx * TP + t, those past NF skipped
    frags = [[w * TP28 + t for t in range(TP28) if w * TP28 + t < NF28] for w in range(WPX28)]
    assert [len(g) for g in frags] == [7, 6] and sorted(sum(frags, [])) == list(range(NF28))
    seen = set()
    for f in range(NF28):
        for fr in range(16):
            o = 16 * f + fr
            r, c = divmod(o, P28)
            real = c < HW28 and r < ROWS28                       # the epilogue's test
            for dy, dx in TAPS:
                h = o + dy * P28 + dx
                assert 0 <= h < SLOTS28, (f, fr, dy, dx)          # discarded lanes too
                if real:
                    want = (r - 1 + dy, c - 1 + dx)
                    got = staged_pixel(h, P28, HW28, ROWS28)
                    assert got == (want if 0 <= want[1] < HW28 else None), (o, dy, dx)
            if real:
                assert (r, c) not in seen
                seen.add((r, c))
    assert len(seen) == ROWS28 * HW28 == 196
    assert 16 * NF28 - 1 + 2 * P28 + 2 == SLOTS28 - 1
