"""The definition of the in-engine dropout draws, checked without a GPU on its numpy restatement tests/dropout_reference.py
— the kernels are compared with that restatement bit for bit in test_dropout_gpu.py."""
import numpy as np
import pytest

from tests import dropout_reference as D

SEED, OFFSET = 0x9E3779B97F4A7C15, (3 << 32) | 0xFFFFFFF8  # both halves of both words in use


def test_known_answer_anchor():
    """seed 0, offset 0, site 0: the counter is (0, 0, 0, 0) under key (0, 0), the Random123 zero vector
    6627E8D5 E169C58D BC57AC4C 9B00DBD8.  u24 = 6627E8 E169C5 BC57AC 9B00DB.  p = 0.3: float32(0.3) * 2^24 = 5033165 = 4CCCCD
    exactly, below all four -> kept, kept, kept, kept.  p = 0.5: the threshold is 800000 -> dropped, kept, kept, kept."""
    assert [int(v) for v in D.words(0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert D.dropout2d_u24(0, 1, 4, 0, 0).tolist() == [[0x6627E8, 0xE169C5, 0xBC57AC, 0x9B00DB]]
    assert D.threshold(0.3) == 0x4CCCCD and D.threshold(0.5) == 0x800000
    k3, k5 = np.float32(1) / np.float32(0.7), np.float32(2)
    assert D.kept_value(0.3) == k3 and D.kept_value(0.5) == k5 and float(k3) == 1.4285714626312256
    assert D.dropout2d_mask(0, 1, 4, 0.3, 0, 0).tolist() == [[k3, k3, k3, k3]]
    assert D.dropout2d_mask(0, 1, 4, 0.5, 0, 0).tolist() == [[0.0, k5, k5, k5]]
    assert D.dropout2d_mask(0, 2, 2, 0.5, 0, 0).tolist() == [[0.0, k5], [k5, k5]]  # flat [N][C]: rows share a counter
    # the first lane group of an element-wise site at pixel 0 of image 0 is the same counter when the site number is 0
    assert D.elem_mask(0, 1, 4, 1, 1, 0.5, 0, 0).reshape(-1).tolist() == [0.0, k5, k5, k5]


def test_index_maps_element_by_element():
    """The vectorised maps against the definition written as loops, at a shape with both tails: N C = 10 = 2 mod 4, and
    C = 6 of pad8 = 8 (the second lane group half used)."""
    n, c, h, w, site = 2, 5, 2, 3, 7
    u = D.dropout2d_u24(site, n, c, SEED, OFFSET)
    for e in range(n * c):
        assert int(u[e // c, e % c]) == int(D.words(e // 4, 0, site, SEED, OFFSET)[e % 4]) >> 8
    c = 6
    u = D.elem_u24(site, n, c, h, w, SEED, OFFSET)
    assert u.shape == (n, c, h, w)
    for ni in range(n):
        for ci in range(c):
            for r in range(h * w):
                word = D.words(r, ni * 2 + ci // 4, site, SEED, OFFSET)[ci % 4]
                assert int(u[ni, ci, r // w, r % w]) == int(word) >> 8
    # and the counter itself: word 2 carries the site in bits 24.., word 3 the offset's high half, the key the seed
    want = D.P.philox4x32_10(5, 9, 0xFFFFFFF8 ^ (7 << 24), 3, 0x7F4A7C15, 0x9E3779B9)
    assert [int(v) for v in D.words(5, 9, 7, SEED, OFFSET)] == [int(v) for v in want]
    assert D.counter_word2(255, 0) == 0xFF000000 and D.counter_word2(256, 5) == 5  # mod 2^32


@pytest.mark.parametrize("p", [0.05, 0.1, 0.2, 0.3, 0.5, 0.9])
def test_float_keep_test_is_the_integer_threshold(p):
    t = D.threshold(p)
    u = np.array(sorted({0, (1 << 24) - 1} | {t + d for d in range(-2, 3)}), dtype=np.uint64)
    assert 2 < t < (1 << 24) - 3
    assert np.array_equal(D.keep_float(u, p), D.keep_int(u, p))
    assert not D.keep_float(np.uint64(t - 1), p) and D.keep_float(np.uint64(t), p)
    assert not D.keep_int(0, p) and D.keep_int((1 << 24) - 1, p)


def _keys(table, offset):
    """(word 2, i0, i1, lane) of every multiplier in use, one row each."""
    rows = []
    for t in table:
        i0, i1, lane = D.used_counters(t)
        rows.append(np.stack([np.full_like(i0, D.counter_word2(t["site"], offset)), i0, i1, lane], axis=1))
    return np.concatenate(rows)


@pytest.mark.parametrize("s,f,n", [(2, 6, 3), (12, 1, 2)], ids=["S2", "S12-the-most-sites"])
def test_no_multiplier_shares_its_randomness_within_one_forward(s, f, n):
    table = D.sites(s, f, n, 32, 32, (0.1, 0.3, 0.5), 0.2, 0.05)
    assert len(table) == 4 * s + 7 <= D.MAX_SITES
    if s == 12:
        assert 4 * (s + 1) + 7 > D.MAX_SITES  # S = 13 is refused by the plan
    assert [t["site"] for t in table] == list(range(len(table)))
    keys = _keys(table, OFFSET)
    assert len(keys) == sum(int(np.prod(t["shape"])) for t in table)
    assert len(np.unique(keys, axis=0)) == len(keys)
    # the same statement on the words themselves at the small model: equal counters are the only way to equal 128-bit blocks
    if s == 2:
        blocks = set()
        for t in table:
            i0, i1, _ = D.used_counters(t)
            ctr = np.unique(np.stack([i0, i1], axis=1), axis=0)
            out = np.stack(D.words(ctr[:, 0], ctr[:, 1], t["site"], SEED, OFFSET), axis=1)
            blocks |= {(t["site"],) + tuple(r) for r in out.tolist()}
            assert len({tuple(r) for r in out.tolist()}) == len(ctr)
        assert len({b[1:] for b in blocks}) == len(blocks)


def test_steps_below_the_first_reuse_offset_are_disjoint():
    """Arithmetic, not enumeration.  (1) no site number reaches below bit 24 of counter word 2, so word 2 mod 2^24 is the
    offset mod 2^24 for every site; (2) offsets o < o' < 2^24 differ mod 2^24 (they ARE their residues), so the two steps share
    no counter whatever their sites — o' = o + 4 in particular; (3) at 2^24 the statement ends: site 1 there is site 0 of
    offset 0."""
    low = (1 << 24) - 1
    assert all((site << 24) & low == 0 for site in range(D.MAX_SITES)) and (D.MAX_SITES - 1) << 24 <= 0xFFFFFFFF  # (1)
    probe = [0, 4, 8, 0x00FFFFF8, 0x00FFFFFC, 0x7FFFFFFC, 0xFFFFFFF8, 0xFFFFFFFC, OFFSET, OFFSET + 4, (1 << 63) + 0x123454]
    for o in probe:
        assert all(D.counter_word2(site, o) & low == o & low for site in range(D.MAX_SITES))
    assert D.FIRST_REUSE_OFFSET == low + 1 and 4 % D.FIRST_REUSE_OFFSET != 0  # (2): o + 4 is another residue, o + 4 <= low or not
    for o in (0, 4, low - 7, low - 3):  # ... spot checks, the last step below the bound included (o + 4 = 2^24 wraps to residue 0)
        a = {D.counter_word2(site, o) for site in range(D.MAX_SITES)}
        b = {D.counter_word2(site, o + 4) for site in range(D.MAX_SITES)}
        assert len(a) == len(b) == D.MAX_SITES and not a & b
    # (3) the first reuse
    assert D.counter_word2(1, D.FIRST_REUSE_OFFSET) == D.counter_word2(0, 0)
    assert np.array_equal(D.dropout2d_u24(1, 2, 8, SEED, D.FIRST_REUSE_OFFSET), D.dropout2d_u24(0, 2, 8, SEED, 0))
    step0 = {D.counter_word2(b, 0) for b in range(D.MAX_SITES)}
    assert not any(D.counter_word2(a, o) in step0 for o in range(4, 4096, 4) for a in range(D.MAX_SITES))


@pytest.mark.parametrize("what", ["seed", "offset"])
def test_both_halves_of_seed_and_offset_are_used(what):
    seed2, offset2 = (SEED ^ (1 << 32), OFFSET) if what == "seed" else (SEED, OFFSET ^ (1 << 32))
    for t in D.sites(2, 6, 3, 32, 32, (0.5, 0.5, 0.5), 0.5, 0.5):
        a, b = D.site_mask(t, SEED, OFFSET), D.site_mask(t, seed2, offset2)
        differ = float((a != b).mean())
        assert 0.25 < differ < 0.75 or a.size < 64 and differ > 0, (t, differ)  # independent masks at p = 0.5 differ in half
    # and the low halves
    t = D.sites(2, 6, 3, 32, 32, final=0.5)[-1]
    assert not np.array_equal(D.site_mask(t, SEED, OFFSET), D.site_mask(t, SEED ^ 1, OFFSET))
    assert not np.array_equal(D.site_mask(t, SEED, OFFSET), D.site_mask(t, SEED, OFFSET ^ 4))


def _corr(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("p", [0.05, 0.3, 0.5])
def test_keep_rate_and_independence(p):
    """2^20 draws per site.  Keep rate within 5 sigma of 1 - float32(p) (sigma = sqrt(p (1 - p) / n)); the correlation of the
    keep indicators of two sites, of two lanes of one counter, and of neighbouring counters within 5 / sqrt(n)."""
    n, c, h, w = 8, 8, 128, 128
    a = D.keep_int(D.elem_u24(20, n, c, h, w, SEED, OFFSET), p)
    b = D.keep_int(D.elem_u24(21, n, c, h, w, SEED, OFFSET), p)
    d2 = D.keep_int(D.dropout2d_u24(3, 1024, 1024, SEED, OFFSET), p)
    for m in (a, b, d2):
        assert m.size == 1 << 20
        rate, sigma = float(m.mean()), (p * (1 - p) / m.size) ** 0.5
        print(f"p = {p}: keep rate {rate:.5f}, {abs(rate - (1 - float(np.float32(p)))) / sigma:.2f} sigma")
        assert abs(rate - (1 - float(np.float32(p)))) < 5 * sigma
    bound = 5 / a.size ** 0.5
    assert abs(_corr(a, b)) < bound and abs(_corr(a.reshape(-1)[:d2.size], d2)) < bound
    lanes = a.reshape(n, 2, 4, h * w)
    lb = 5 / lanes[:, :, 0].size ** 0.5
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(_corr(lanes[:, :, i], lanes[:, :, j])) < lb, (i, j)
    assert abs(_corr(lanes[..., :-1], lanes[..., 1:])) < 5 / lanes[..., 1:].size ** 0.5  # counters i0 and i0 + 1
    assert abs(_corr(lanes[:, 0], lanes[:, 1])) < 5 / lanes[:, 0].size ** 0.5           # counters i1 and i1 + 1


def test_boundary_constants_hit_u_equal_p_exactly():
    """The committed (seed, offset, site, geometry, index) has u24 = 2^23: float32(u24) * 2^-24 == 0.5 == p, kept by `>=`.
    The search that produced it is replayed over its last stretch (it stops at its first hit, which is the constant)."""
    g = D.BOUNDARY_GEOMETRY
    table = D.sites(g["s"], g["f"], g["n"], g["h"], g["w"], final=0.5)
    t = table[D.BOUNDARY_SITE]
    assert t["kind"] == "final1" and t["shape"] == (1, 6, 32, 32)
    u = D.site_u24(t, D.BOUNDARY_SEED, D.BOUNDARY_OFFSET)
    assert int(u[D.BOUNDARY_INDEX]) == 1 << 23 == D.threshold(0.5)
    assert np.float32(int(u[D.BOUNDARY_INDEX])) * np.float32(2.0 ** -24) == np.float32(0.5)
    assert D.site_mask(t, D.BOUNDARY_SEED, D.BOUNDARY_OFFSET)[D.BOUNDARY_INDEX] == np.float32(2.0)
    assert D.BOUNDARY_SITE == D.num_double_convs(g["s"]) + 2 and D.BOUNDARY_OFFSET % 4 == 0
    assert D.BOUNDARY_OFFSET >> 32 and D.BOUNDARY_SEED >> 32  # both high words in use on the device too
    found = D.search_boundary(D.BOUNDARY_SEED, **g, max_offsets=64, start_offset=D.BOUNDARY_OFFSET - 4 * 60)
    assert found == (D.BOUNDARY_OFFSET, D.BOUNDARY_SITE, D.BOUNDARY_INDEX)
    assert (D.BOUNDARY_OFFSET - D.BOUNDARY_SEARCH_START) // 4 == 1215
