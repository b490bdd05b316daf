"""The board lists of tests/test_gpu_board_lists_dev_blocks.py: device lists longer than one
block of the check kernel (csrc/td_list_check.hip: one thread per entry, kListCheckThreads = 256
to a block).  No GPU, no torch: tests/test_list_cases_host.py checks this table on any machine.

B = 2,100 boards, so cap = B gives 9 check blocks: block k holds entries [256 k, 256 k + 256),
blocks 0-7 fall on eight different XCDs and block 8 on block 0's (the project's own assumption,
NXCD in csrc/td_kernels.h: block i runs on XCD i % 8 -- assumed, never asserted), and the last
block is partial and shorter than a wave (entries 2,048-2,099).

A row is one device call: its kind ("step", "mask", "copy+" = a copy with write_obs, "copy-" =
without), the buffers src (None but for a copy) and dst of cap entries, the count (None = no
count_dev), the code the hand-made rows expect (None for a random row: listref decides), and for
a refused row the valid follow-up (src, dst) that names the same boards."""
import collections

import numpy as np

import listref as R

B = 2100
BLOCK = 256  # kListCheckThreads
NXCD = 8
OK, BAD_COUNT, RANGE, TWICE, OVERLAP = R.OK, R.BAD_COUNT, R.RANGE, R.TWICE, R.OVERLAP
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
POISON = (-7, B + 5)

Row = collections.namedtuple("Row", "name kind src dst count cap code follow")


def used(row):
    """How many entries the row's call reads as ids (0 for a bad count)."""
    n = row.cap if row.count is None else row.count
    return n if 0 <= n <= row.cap else 0


def expect(row):
    return R.verdict(row.src, row.dst, row.count, row.cap, B)


# ------------------------------------------------------------------ valid lists
def step_list(n, seed):
    """n distinct boards in a seeded order, and the boards left over."""
    p = np.random.RandomState(seed).permutation(B).tolist()
    return p[:n], p[n:]


def copy_lists(n, seed, roots=0):
    """A valid copy of n pairs: distinct destinations; the sources are boards that are no
    destination -- all distinct while 2 n <= B, else the free boards in turn (so no two lanes of
    a wave name one source while 64 are free); roots > 0: a fan-out of that many roots."""
    p = np.random.RandomState(seed).permutation(B).tolist()
    if roots:
        assert n + roots <= B
        free, dst = p[:roots], p[roots:roots + n]
    else:
        assert n < B
        dst, free = p[:n], p[n:]
    src = [free[i % len(free)] for i in range(n)]
    return src, dst, free[n:]  # (the boards named by neither list; none once the free ones go round)


def _unique_valid(ids):
    seen, out = set(), []
    for x in ids:
        if 0 <= x < B and x not in seen:
            seen.add(x)
            out.append(x)
    return out


def _row(name, kind, src, dst, count, cap, code, base=None):
    """base: the valid (src, dst) the defect was planted in: a copy's follow-up.  A step's or
    mask's is the distinct valid ids the bad list used."""
    assert len(dst) == cap and (src is None) == (not kind.startswith("copy")) and (src is None or len(src) == cap)
    row = Row(name, kind, src, dst, count, cap, code, None)
    if code == OK:
        return row
    if src is None:
        n = used(row) or cap
        follow = (None, _unique_valid(dst[:n]))
    else:
        follow = base
    return row._replace(follow=follow)


# ------------------------------------------------------------------ the hand-made table
def hand_rows():
    rows = []
    seed = [100]

    def fresh():
        seed[0] += 1
        return seed[0]

    def alt(i, kinds):
        return kinds[i % len(kinds)]

    # ---- TWICE in a step / mask list, cap = B: the pair's positions
    pairs = [((3, 40), "same wave"), ((3, 200), "same block, other wave"), ((255, 256), "adjacent blocks"),
             ((10, 1300), "blocks 0 and 5"), ((10, 2060), "blocks 0 and 8: one XCD, the second in the partial block"),
             ((2050, 2099), "both in the partial block"), ((5, 700, 1900), "a triple")]
    for k, (pos, what) in enumerate(pairs):
        dst, _ = step_list(B, fresh())
        for q in pos[1:]:
            dst[q] = dst[pos[0]]
        rows.append(_row("twice %s (%s)" % (pos, what), alt(k, ("step", "mask")), None, dst, None, B, TWICE))

    # ---- TWICE in a copy's dst.  (255, 256): 1,000 pairs, every source distinct.  (10, 1300):
    # 1,400 pairs need 1,399 + 1,400 boards if every source were distinct too, more than B: the
    # 700 free boards serve as sources in turn, distinct within every wave.
    for k, (pos, n) in enumerate((((255, 256), 1000), ((10, 1300), 1400))):
        src, dst, _ = copy_lists(n, fresh())
        base = (list(src), list(dst))
        dst[pos[1]] = dst[pos[0]]
        if n == 1000:
            assert len(set(src)) == n
        rows.append(_row("copy twice %s" % (pos,), alt(k, ("copy+", "copy-")), src, dst, None, n, TWICE, base))

    # ---- OVERLAP (a copy): the source entry, the destination entry
    for k, (si, di, n, what) in enumerate([(20, 1600, 1700, "source block 0, destination block 6"),
                                           (1600, 20, 1700, "source block 6, destination block 0"),
                                           (255, 256, 1000, "adjacent blocks"),
                                           (2060, 10, 2090, "blocks 8 and 0: one XCD"),
                                           (2050, 2085, 2090, "both in the partial block")]):
        src, dst, _ = copy_lists(n, fresh())
        base = (list(src), list(dst))
        dst[di] = src[si]
        rows.append(_row("overlap src[%d] dst[%d] (%s)" % (si, di, what), alt(k, ("copy+", "copy-")), src, dst, None, n,
                         OVERLAP, base))
    # the full fan-out: 2,099 children of one root, and the root is entry 1,500's destination
    src, dst, _ = copy_lists(B - 1, fresh(), roots=1)
    base = (list(src), list(dst))
    dst[1500] = src[0]
    rows.append(_row("overlap fan-out: the root is dst[1500]", "copy-", src, dst, None, B - 1, OVERLAP, base))
    # a whole wave of block 5 names X as its source; only one lane of it does (the s != s0 path)
    for k, lanes in enumerate((range(1280, 1344), (1297,))):
        src, dst, spare = copy_lists(690, fresh())  # (720 boards to spare)
        src, dst = src + src + src[:20], dst + spare[:710]  # 1,400 pairs: sources twice, no destination among them
        x = spare[-1]
        for i in lanes:
            src[i] = x
        base = (list(src), list(dst))
        dst[7] = x
        rows.append(_row("overlap: %s of wave 20 names dst[7]" % ("all 64 lanes" if k == 0 else "lane 17 alone"),
                         alt(k, ("copy+", "copy-")), src, dst, None, 1400, OVERLAP, base))

    # ---- RANGE
    for k, (kind, v) in enumerate((("step", B), ("mask", -1))):
        dst, _ = step_list(B, fresh())
        dst[B - 1] = v
        rows.append(_row("range dst[2099] = %d" % v, kind, None, dst, None, B, RANGE))
    for kind in ("step", "mask"):  # two at once: the lower entry is the one reported
        dst, _ = step_list(B, fresh())
        dst[1900], dst[300] = B + 1, -2
        rows.append(_row("range at 1900 and at 300 (%s)" % kind, kind, None, dst, None, B, RANGE))
    for k, (what, plant) in enumerate([
            ("src[256] = 2**31 - 1", lambda s, d: s.__setitem__(256, INT_MAX)),
            ("src[1344] (lane 0 of its wave) = B", lambda s, d: s.__setitem__(1344, B)),
            ("src[700] and dst[700]", lambda s, d: (s.__setitem__(700, -1), d.__setitem__(700, B + 9))),
            ("dst[2088] = -2**31", lambda s, d: d.__setitem__(2088, INT_MIN))]):
        n = 2090 if "2088" in what else 1400
        src, dst, _ = copy_lists(n, fresh())
        base = (list(src), list(dst))
        plant(src, dst)
        rows.append(_row("copy range " + what, alt(k, ("copy+", "copy-")), src, dst, None, n, RANGE, base))

    # ---- the lowest code wins, across blocks
    dst, _ = step_list(B, fresh())
    dst[30] = dst[5]  # TWICE in block 0
    dst[2070] = B  # RANGE in block 8
    rows.append(_row("range in block 8 over twice in block 0", "step", None, dst, None, B, RANGE))
    src, dst, _ = copy_lists(2000, fresh())
    base = (list(src), list(dst))
    dst[40] = src[9]  # OVERLAP in block 0
    dst[1900] = dst[1800]  # TWICE in block 7
    rows.append(_row("twice in block 7 over overlap in block 0", "copy+", src, dst, None, 2000, TWICE, base))
    dst, _ = step_list(B, fresh())
    for i in range(1, B, 2):
        dst[i] = dst[i - 1]
    rows.append(_row("bad count over a list full of duplicates", "mask", None, dst, B + 1, B, BAD_COUNT))

    # ---- BAD_COUNT, cap = B: every count with every kind
    k = 0
    for count in (-1, B + 1, INT_MAX, INT_MIN):
        for kind in ("step", "mask", "copy"):
            if kind == "copy":
                kind = alt(k, ("copy+", "copy-"))
                k += 1
                src, dst, _ = copy_lists(1000, fresh())
                base = (list(src), list(dst))
                pad = B - 1000
                src, dst = src + [POISON[0]] * pad, dst + [dst[0]] * pad
                rows.append(_row("bad count %d (%s)" % (count, kind), kind, src, dst, count, B, BAD_COUNT, base))
            else:
                dst, _ = step_list(B, fresh())
                rows.append(_row("bad count %d (%s)" % (count, kind), kind, None, dst, count, B, BAD_COUNT))

    # ---- counts that must be accepted, cap = B, poison behind them: duplicates of used ids, -7,
    # B + 5.  "near": the poison fills the rest of the block that holds entry `count`; "far": only
    # the blocks wholly behind that one; everything else behind the count is unused valid ids.
    kinds = ("step", "mask", "copy+", "copy-")
    k = 0
    for count in (0, 1, 10, 255, 256, 257, 2047, 2048, 2049, 2099, 2100):
        edge = min(B, BLOCK * (count // BLOCK + 1))
        for where, lo, hi in (("near", count, edge), ("far", edge, B)):
            if lo >= hi:
                continue
            kind = alt(k, kinds if count < B else kinds[:2])  # (no copy names all B boards as destinations)
            k += 1
            src, dst = _counted(kind, count, fresh())
            for i in range(lo, hi):
                v = (dst[i % count] if count else 0, POISON[0], POISON[1])[i % 3]
                dst[i] = v
                if src is not None:
                    src[i] = (POISON[1], dst[(i + 1) % count] if count else 0, POISON[0])[i % 3]
            rows.append(_row("count %d, poison %s [%d, %d) (%s)" % (count, where, lo, hi, kind), kind, src, dst, count, B,
                             OK))
        if count == B:  # (no room for poison: the plain list)
            for kind in ("step", "mask"):
                rows.append(_row("count %d = cap (%s)" % (count, kind), kind, None, _counted(kind, count, fresh())[1], count,
                                 B, OK))
        # a duplicate of entry 0 as the last entry used, and as the first one not used
        if count >= 1:
            kind = alt(k, kinds if count < B else kinds[:2])  # (no copy names all B boards as destinations)
            k += 1
            src, dst = _counted(kind, count, fresh())
            base = None if src is None else (src[:count], dst[:count])
            dst[count - 1] = dst[0]
            rows.append(_row("count %d, dst[%d] = dst[0] (%s)" % (count, count - 1, kind), kind, src, dst, count, B,
                             TWICE if count >= 2 else OK, base))
        if count < B:
            kind = alt(k, kinds if count < B else kinds[:2])  # (no copy names all B boards as destinations)
            k += 1
            src, dst = _counted(kind, count, fresh())
            dst[count] = dst[0]
            rows.append(_row("count %d, dst[%d] = dst[0]: not used (%s)" % (count, count, kind), kind, src, dst, count, B, OK))

    # ---- cap below B without a count: a partial last check block and no count_dev
    for k, cap in enumerate((257, 1000, 2099)):
        kind = alt(k, ("step", "copy+", "mask"))
        if kind == "copy+":
            src, dst, _ = copy_lists(cap, fresh())
        else:
            src, dst = None, step_list(cap, fresh())[0]
        rows.append(_row("cap %d, no count (%s)" % (cap, kind), kind, src, dst, None, cap, OK))
    return rows


def _counted(kind, count, seed):
    """Buffers of B entries whose first `count` are a valid list of `kind`; behind them unused
    valid ids (a copy: sources in range)."""
    if not kind.startswith("copy"):
        return None, step_list(B, seed)[0]
    n = count
    assert n < B  # (a copy cannot name every board as a destination)
    src, dst, _ = copy_lists(n, seed, roots=0 if 2 * n <= B else 1) if n else ([], [], [])
    named = set(dst)
    rest = [x for x in np.random.RandomState(seed).permutation(B).tolist() if x not in named]
    pad = B - n
    return src + [rest[i % len(rest)] for i in range(pad)], dst + [rest[(i + 1) % len(rest)] for i in range(pad)]


# ------------------------------------------------------------------ the seeded random rows
def random_rows(count=24, seed=20261):
    rng = np.random.RandomState(seed)
    rows = []
    for r in range(count):
        kind = ("step", "mask", "copy+", "copy-")[int(rng.randint(4))]
        fan = r % 3 == 0
        if fan:
            kind = ("copy+", "copy-")[r // 3 % 2]
        copy = kind.startswith("copy")
        roots = int(rng.randint(1, 4)) if fan else 0
        n = int(rng.randint(257, B + 1 - (max(roots, 1) if copy else 0)))
        s = int(rng.randint(1 << 30))
        if copy:
            src, dst, _ = copy_lists(n, s, roots=roots)
            if roots > 1:
                src = [src[int(j)] for j in rng.randint(0, n, size=n)]  # the roots in a random order
        else:
            src, dst = None, step_list(n, s)[0]
        base = None if src is None else (list(src), list(dst))
        edges = [e for e in (0, 63, 64, 255, 256, 2047, 2048, n - 1) if e < n]

        def pos():
            return int(edges[rng.randint(len(edges))]) if rng.randint(2) else int(rng.randint(n))

        for _ in range(int(rng.randint(0, 4))):
            code = (RANGE, TWICE, OVERLAP)[int(rng.randint(3 if copy else 2))]
            p, q = pos(), pos()
            if code == RANGE:
                v = (-1, B, B + 5, INT_MAX, INT_MIN)[int(rng.randint(5))]
                (src if copy and rng.randint(2) else dst)[p] = v
            elif p != q and code == TWICE:
                dst[q] = dst[p]
            elif code == OVERLAP:
                dst[q] = src[p]
        cap, cnt = n, None
        if rng.randint(2):  # through count_dev, with poison behind the count
            cap, cnt = B, n
            pad = [(dst[i % n], POISON[0], POISON[1])[i % 3] for i in range(B - n)]
            dst = dst + pad
            if copy:
                src = src + pad[::-1]
        code = R.verdict(src, dst, cnt, cap, B)[0]
        rows.append(_row("random %d (%s%s, n = %d)" % (r, kind, ", %d roots" % roots if fan else "", n), kind, src, dst,
                         cnt, cap, code, base)._replace(code=None))
    return rows


_TABLE = []


def table():
    if not _TABLE:
        _TABLE.extend(hand_rows() + random_rows())
    return list(_TABLE)


# ------------------------------------------------------------------ what the table covers
def conflict_pairs(row):
    """The pairs of used entries (i, j) whose meeting on one mark word is the row's verdict:
    two destinations of one board (TWICE), a source and a destination (OVERLAP).  Of a board that
    more than 8 sources name, only its lowest and its highest source entry are paired."""
    code = expect(row)[0]
    n = used(row)
    at = collections.defaultdict(list)
    for i, d in enumerate(row.dst[:n]):
        at[d].append(i)
    pairs = []
    if code == TWICE:
        for e in at.values():
            pairs += [(e[x], e[y]) for x in range(len(e)) for y in range(x + 1, len(e))]
    elif code == OVERLAP:
        by = collections.defaultdict(list)
        for i, s in enumerate(row.src[:n]):
            if s in at:
                by[s].append(i)
        for s, e in by.items():
            e = e if len(e) <= 8 else [e[0], e[-1]]
            pairs += [(i, j) for i in e for j in at[s]]
    return pairs


def coverage(rows):
    """Counts over rows: the rows per verdict code; the conflict pairs whose two entries lie in
    different check blocks, split by whether the blocks share an XCD residue (block % NXCD); the
    refused rows with an entry the device may report inside a partial last block of the grid."""
    per_code = collections.Counter()
    cross = same = other = partial = 0
    for row in rows:
        code, allowed = expect(row)
        per_code[code] += 1
        for i, j in conflict_pairs(row):
            bi, bj = i // BLOCK, j // BLOCK
            if bi != bj:
                cross += 1
                if bi % NXCD == bj % NXCD:
                    same += 1
                else:
                    other += 1
        tail = BLOCK * (row.cap // BLOCK)
        if code != OK and row.cap % BLOCK and any(e >= tail for e, _ in allowed):
            partial += 1
    return dict(rows_per_code=dict(per_code), accepted=per_code[OK], cross_block_pairs=cross, same_xcd_pairs=same,
                other_xcd_pairs=other, partial_block_rows=partial)
