"""The grab schedule of the walk kernel's dynamic work loop (ugs_kernels.hip, ugs_walk_lds, `if (a.work_next)`), restated in plain Python.

A launch of `total` items runs on `groups` waves.  The device counter counts items.  A wave takes its first grab by its index; every
further one by atomicAdd(counter, size) with a size chosen from what the wave believes is left -- `total` minus its OWN position,
which is at or behind the counter -- by the ladder

    GRAB  while more than 2 * GRAB items per group are left
    4     while more than 8 per group are left
    2     while more than 2 per group are left
    1     for the rest

(the one-walk-per-wave tiers; the 8- and 16-lane tiers keep the ladder without its first step).  A grab is worked off as sub-chunks of at most CHUNK = 4 consecutive rows (a DPP row of the wave per walk: chunk_draws, Parked); a
grab cut short by `total` ends inside a sub-chunk.  Which wave takes a row changes no result: row i depends on (seed, i) alone."""
CHUNK = 4
GRAB = 32                      # UGS_WORK_GRAB
WAVES_PER_CU = 20              # UGS_BLOCKS_M: resident one-wave blocks per compute unit in the 448-candidate tier
DYNAMIC_ABOVE_PER_CU = 64      # the host takes the dynamic loop above this many rows per compute unit


def grab_for(left, groups):
    if left > 2 * GRAB * groups:
        return GRAB
    return 4 if left > 8 * groups else (2 if left > 2 * groups else 1)


def sub_chunks(lo, hi):
    """the sub-chunks [a, b) a wave works a grab [lo, hi) off as"""
    out = []
    while lo < hi:
        out.append((lo, min(lo + CHUNK, hi)))
        lo = out[-1][1]
    return out


def schedule(total, groups, rng=None):
    """Every grab of a launch, in the order the grabs were made: (wave, lo, hi, size asked for, from the counter?), [lo, hi) already
    cut by `total` (empty grabs are left out: a wave that finds the counter past the end returns).  The order in which the waves
    come back to the counter is what the model cannot know: in turn without `rng` (a launch whose walks all cost the same), else
    the next wave drawn by `rng` among those still running."""
    first = grab_for(total, groups)
    grabs, pos, counter = [], {}, 0
    for w in range(groups):                                   # the kernel: it = group * first, gend = it + first, while (it < total)
        lo = w * first
        if lo < total:
            hi = min(lo + first, total)
            grabs.append((w, lo, hi, first, False))
            pos[w] = hi
    running, turn = list(pos), 0
    while running:
        i = rng.randrange(len(running)) if rng else turn % len(running)
        w = running[i]
        size = grab_for(total - pos[w], groups)               # chunk_for(total - it), `it` at the end of the wave's last grab
        lo = groups * first + counter
        counter += size
        if lo < total:
            hi = min(lo + size, total)
            grabs.append((w, lo, hi, size, True))
            pos[w] = hi
            turn = i + 1
        elif rng:
            running[i] = running[-1]
            running.pop()
        else:
            running.pop(i)                                    # the next wave in turn moves into place i
            turn = i
    return grabs


def sizes_reached(total, groups):
    """{size asked for: grabs of it that hand out at least one row} with the waves coming back in turn"""
    seen = {}
    for _, lo, hi, size, _ in schedule(total, groups):
        seen[size] = seen.get(size, 0) + 1
    return seen


def is_dynamic(rows, cus):
    return rows > cus * DYNAMIC_ABOVE_PER_CU


def full_residency_rows(cus):
    """case (ii): just over 2 * GRAB rows per resident wave, plus 13 -- the first grab of every wave is GRAB rows"""
    return 2 * GRAB * cus * WAVES_PER_CU + 13
