"""tests/listref.py and tests/listcases.py without a GPU: the reference of a device-list verdict on
lists whose answer is obvious, against a brute-force restatement of the header's sentences
(include/tdstep.h, above enum td_list_code) over every small list, and the conditions the case
table of tests/test_gpu_board_lists_dev_blocks.py must meet before it is worth a GPU run."""
import itertools

import pytest

import listcases as C
import listref as R

OK, BAD_COUNT, RANGE, TWICE, OVERLAP = R.OK, R.BAD_COUNT, R.RANGE, R.TWICE, R.OVERLAP


@pytest.mark.parametrize("src,dst,count,cap,B,code,allowed", [
    (None, [0, 1, 2], None, 3, 3, OK, set()),
    (None, [], None, 0, 3, OK, set()),
    (None, [2, 2, 2], 0, 3, 3, OK, set()),  # nothing is used
    (None, [0, 1, 0], 2, 3, 3, OK, set()),  # the duplicate lies behind the count
    (None, [0, 1, 0], 3, 3, 3, TWICE, {(0, 0), (2, 0)}),
    (None, [0, 1, 0], None, 3, 3, TWICE, {(0, 0), (2, 0)}),
    (None, [0, 9, -1], None, 3, 3, RANGE, {(1, 9)}),  # the lowest entry
    (None, [0, 3, 0], None, 3, 3, RANGE, {(1, 3)}),  # B itself is outside; RANGE before TWICE
    (None, [7, 7, 7], 4, 3, 3, BAD_COUNT, {(-1, 4)}),
    (None, [7, 7, 7], -1, 3, 3, BAD_COUNT, {(-1, -1)}),
    ([0, 0, 0], [1, 2, 3], None, 3, 4, OK, set()),  # a source repeated: a fan-out
    ([0, 1], [2, 0], None, 2, 3, OVERLAP, {(0, 0), (1, 0)}),
    ([0, 0, 1], [2, 3, 0], None, 3, 4, OVERLAP, {(0, 0), (1, 0), (2, 0)}),
    ([0, 1], [1, 1], None, 2, 3, TWICE, {(0, 1), (1, 1)}),  # TWICE before OVERLAP
    ([5, 1], [-1, 2], None, 2, 3, RANGE, {(0, 5), (0, -1)}),  # both sides of one entry
    ([0, 5], [1, 2], None, 2, 3, RANGE, {(1, 5)}),
    ([2, 2], [2, 1], 1, 2, 3, OVERLAP, {(0, 2)}),  # a pair that copies a board onto itself
])
def test_listref_on_obvious_lists(src, dst, count, cap, B, code, allowed):
    assert R.verdict(src, dst, count, cap, B) == (code, allowed)


def _brute(src, dst, count, cap, B):
    """The header's sentences, one at a time, as set comprehensions over the used entries."""
    n = cap if count is None else count
    if not 0 <= n <= cap:  # "a count outside [0, cap]"; "entry is -1 and board the count read"
        return BAD_COUNT, {(-1, n)}
    use = range(n)  # "the first *count_dev entries are used"
    lists = [dst] if src is None else [src, dst]
    outside = {(i, l[i]) for l in lists for i in use if not 0 <= l[i] < B}  # "an id outside [0, boards)"
    if outside:
        low = min(i for i, _ in outside)  # (each entry shows its own id: the lowest is reported)
        return RANGE, {(i, x) for i, x in outside if i == low}
    twice = {(i, dst[i]) for i in use for j in use if i != j and dst[i] == dst[j]}  # "a board named twice in boards or in dst"
    if twice:
        return TWICE, twice  # "any one of the entries that name the board"
    if src is not None:
        both = {src[i] for i in use} & {dst[i] for i in use}  # "a board named in both src and dst"
        over = {(i, l[i]) for l in lists for i in use if l[i] in both}
        if over:
            return OVERLAP, over
    return OK, set()


def test_listref_against_brute_force_on_every_small_list():
    """Every list of at most 3 entries over 4 boards, ids drawn from -1 .. 4 (so both ends of the
    range are passed), as a step list and as a copy, with every count from -1 to cap + 1."""
    B, ids = 4, range(-1, 5)
    codes = set()
    for cap in range(4):
        for dst in itertools.product(ids, repeat=cap):
            for src in [None] + list(itertools.product(ids, repeat=cap)):
                for count in [None] + list(range(-1, cap + 2)):
                    got = R.verdict(src, list(dst), count, cap, B)
                    assert got == _brute(src, dst, count, cap, B), (src, dst, count, cap)
                    codes.add(got[0])
    assert codes == {OK, BAD_COUNT, RANGE, TWICE, OVERLAP}


def test_hand_made_rows_expect_what_listref_says():
    rows = C.hand_rows()
    assert len(set(r.name for r in C.table())) == len(C.table())
    for r in rows:
        assert C.expect(r)[0] == r.code, (r.name, r.code, C.expect(r))


def test_every_row_is_well_formed():
    for r in C.table():
        code, allowed = C.expect(r)
        assert r.kind in ("step", "mask", "copy+", "copy-") and r.cap <= C.B and len(r.dst) == r.cap, r.name
        assert (r.src is not None) == r.kind.startswith("copy"), r.name
        assert all(-2 ** 31 <= x < 2 ** 31 for l in (r.src or [], r.dst) for x in l), r.name
        if code == OK:
            assert r.follow is None and not allowed, r.name
            continue
        # a refused row's follow-up is valid, and names boards the refused list named
        fs, fd = r.follow
        assert R.verdict(fs, fd, None, len(fd), C.B) == (OK, set()), r.name
        assert (fs is not None) == (r.src is not None) and 0 < len(fd) <= r.cap, r.name
        named = set(r.dst) | set(r.src or [])
        assert len(set(fd) & named) >= len(fd) - 3, r.name  # (but for the few entries a defect was planted in)


def test_the_table_covers_what_it_is_for():
    rows = C.table()
    assert len(C.random_rows()) == 24
    cov = C.coverage(rows)
    for code in (BAD_COUNT, RANGE, TWICE, OVERLAP):
        assert cov["rows_per_code"].get(code, 0) >= 8, (R.NAMES[code], cov)
    assert cov["accepted"] >= 12, cov
    assert cov["cross_block_pairs"] >= 10 and cov["same_xcd_pairs"] >= 3 and cov["other_xcd_pairs"] >= 3, cov
    assert cov["partial_block_rows"] >= 4, cov
    # each code refused at least twice by every call that can show it (a step or mask list has no
    # sources, so no OVERLAP); a copy once with write_obs and once without
    per = {}
    for r in rows:
        key = (r.kind, C.expect(r)[0])
        per[key] = per.get(key, 0) + 1
    for code in (BAD_COUNT, RANGE, TWICE):
        assert per.get(("step", code), 0) >= 2 and per.get(("mask", code), 0) >= 2, (R.NAMES[code], per)
    for code in (BAD_COUNT, RANGE, TWICE, OVERLAP):
        assert per.get(("copy+", code), 0) >= 1 and per.get(("copy-", code), 0) >= 1, (R.NAMES[code], per)
    # a mask list of odd length: the last workgroup of four waves is partial
    assert any(r.kind == "mask" and C.used(r) % 2 for r in rows if C.expect(r)[0] == OK)
    assert any(r.kind == "mask" and len(r.follow[1]) % 4 for r in rows if r.follow)


def test_the_named_positions_are_in_the_table():
    """The rows the case table is built around, found by what they hold."""
    rows = C.hand_rows()

    def twice_at(kinds, pos):
        for r in rows:
            if r.kind in kinds and r.count is None and C.expect(r)[0] == TWICE and \
                    sorted(e for e, _ in C.expect(r)[1]) == list(pos):
                return True
        return False

    for pos in ((3, 40), (3, 200), (255, 256), (10, 1300), (10, 2060), (2050, 2099), (5, 700, 1900)):
        assert twice_at(("step", "mask"), pos), pos
    for pos in ((255, 256), (10, 1300)):
        assert twice_at(("copy+", "copy-"), pos), pos
    fan = [r for r in rows if r.src and len(set(r.src)) == 1 and r.cap == C.B - 1]
    assert fan and fan[0].dst[1500] == fan[0].src[0] and C.expect(fan[0])[0] == OVERLAP
    for count in (-1, C.B + 1, 2 ** 31 - 1, -2 ** 31):
        assert any(r.count == count and r.cap == C.B for r in rows), count
    for count in (0, 1, 10, 255, 256, 257, 2047, 2048, 2049, 2099, 2100):
        assert sum(1 for r in rows if r.count == count and r.cap == C.B and C.expect(r)[0] == OK) >= 2, count
        if count >= 2:
            assert any(r.count == count and C.expect(r) == (TWICE, {(0, r.dst[0]), (count - 1, r.dst[0])}) for r in rows), count
    for cap in (257, 1000, 2099):
        assert any(r.cap == cap and r.count is None and C.expect(r)[0] == OK for r in rows), cap
