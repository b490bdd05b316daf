"""The plain reference of a device-list verdict (td_step_boards_dev, td_copy_boards_dev,
td_action_mask_boards_dev): which code the check must give for a list, and which (entry, board)
pairs it may report.  Written from the contract in include/tdstep.h (the comment above
enum td_list_code) and the key order of csrc/td_list_check.h ("lowest code wins, then the
lowest entry among those detected") -- not from the kernel: no GPU, no torch, loops only.

An out-of-range id is detected by the entry that holds it, so RANGE reports the lowest such
entry.  A board twice, or in both lists, is detected by whichever of its entries comes second on
the device, so any entry that names the board may be reported."""

OK, BAD_COUNT, RANGE, TWICE, OVERLAP = range(5)
NAMES = ("OK", "BAD_COUNT", "RANGE", "TWICE", "OVERLAP")


def verdict(src, dst, count, cap, B):
    """src: a copy's sources, or None for a step or mask list.  dst: its destinations / the
    boards.  count: None = cap entries.  Returns (code, allowed): allowed is the set of
    (entry, board) pairs the status may hold (empty for OK)."""
    n = cap if count is None else count
    if n < 0 or n > cap:
        return BAD_COUNT, {(-1, n)}
    dst = [int(x) for x in dst[:n]]
    src = None if src is None else [int(x) for x in src[:n]]

    def out(x):
        return x < 0 or x >= B

    for i in range(n):  # the lowest entry with an id out of range, either side
        bad = set()
        if src is not None and out(src[i]):
            bad.add((i, src[i]))
        if out(dst[i]):
            bad.add((i, dst[i]))
        if bad:
            return RANGE, bad

    times = {}
    for d in dst:
        times[d] = times.get(d, 0) + 1
    twice = set((i, d) for i, d in enumerate(dst) if times[d] >= 2)
    if twice:
        return TWICE, twice

    if src is not None:
        both = set(src) & set(dst)
        allowed = set((i, s) for i, s in enumerate(src) if s in both) | set((i, d) for i, d in enumerate(dst) if d in both)
        if allowed:
            return OVERLAP, allowed
    return OK, set()
