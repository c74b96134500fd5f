"""The rooted cyclic-reduction schedule of the one-tile path (no GPU): the crr_* functions of gpmp2_amd/csrc/cr_schedule.h,
which cr_kernels.hip (k_assemble, cr_forward / cr_backward, the finish kernels) and the fused finish of k_linearize_arm
share with their launchers, built by the host compiler (rooted_shim) and checked for every trajectory length.  Blocks
are tree indices v = state + 1 in [1, N + 1]; there is no block 0."""
import rooted_shim as shim

LENGTHS = range(1, 261)


def walk_forward(N, first_level=1):
    """runs the forward levels; -> {v: level it was eliminated at}, [levels]"""
    M, top = N + 1, shim.top(N)
    eliminated_at, levels = {}, []
    h = 1
    while h <= top:
        tasks, (countE, countU) = shim.level(N, h, updates=h > 1)
        assert len(tasks) == countE + countU
        blocks = [v for _, v in tasks]
        # no task names v = 0 or v > N + 1, and none names a block twice
        assert len(set(blocks)) == len(blocks) and all(1 <= v <= M for v in blocks), (N, h)
        for kind, v in tasks:
            assert v % h == 0, (N, h, v)
            if h > 1:   # the neighbours a block absorbs were eliminated one level below
                assert eliminated_at.get(v - h // 2) == h // 2, (N, h, v)
                if v + h // 2 <= M:
                    assert eliminated_at.get(v + h // 2) == h // 2, (N, h, v)
            # its fill-in couplings go to blocks that are still in the tree
            for vn in (v - h, v + h):
                if kind == "E" and 1 <= vn <= M:
                    assert vn not in eliminated_at, (N, h, v, vn)
        for kind, v in tasks:
            if kind == "E":
                assert v not in eliminated_at and (v // h) % 2 == 1, (N, h, v)
                eliminated_at[v] = h
        # the U tasks of a level are exactly the surviving blocks
        if h > 1:
            assert sorted(v for k, v in tasks if k == "U") == [v for v in range(1, M + 1) if v not in eliminated_at], (N, h)
        levels.append(h)
        h <<= 1
    return eliminated_at, levels


def test_every_block_is_eliminated_once_after_the_neighbours_it_absorbs():
    for N in LENGTHS:
        eliminated_at, _ = walk_forward(N)
        assert sorted(eliminated_at) == list(range(1, N + 2)), N
        assert all(h == (v & -v) for v, h in eliminated_at.items()), N     # the level of the lowest set bit


def test_top_level_is_one_block_without_couplings():
    for N in LENGTHS:
        top = shim.top(N)
        assert top & (top - 1) == 0 and top <= N + 1 < 2 * top
        tasks, counts = shim.level(N, top)
        assert tasks == [("E", top)] and counts == (1, 0)
        assert top - top < 1 and top + top > N + 1          # neither coupling exists


def test_level_count_is_one_fewer_than_before_unless_the_tree_is_full():
    for N in LENGTHS:
        _, levels = walk_forward(N)
        assert len(levels) == shim.levels(N) == (N + 1).bit_length() == levels[-1].bit_length()
        old = shim.hfinal(N).bit_length()                    # levels 1 .. hfinal of the schedule that keeps block 0
        assert len(levels) <= old
        assert len(levels) == old - 1 or (N + 1) & N == 0    # N + 1 = 2^k: a full tree has the same depth


def test_backward_order_reads_only_solved_blocks():
    for N in LENGTHS:
        eliminated_at, _ = walk_forward(N)
        solved = set()
        h = shim.top(N)
        while h >= 1:
            count = shim.back_count(N, h)
            new = set()
            for idx in range(count):
                v = shim.back_block(N, h, idx)
                assert eliminated_at[v] == h and v not in solved and v not in new
                for vn in (v - h, v + h):
                    if 1 <= vn <= N + 1:
                        assert vn in solved, (N, h, v, vn)
                new.add(v)
            solved |= new
            h >>= 1
        assert solved == set(range(1, N + 2)), N


def test_one_tile_kernels_split_the_levels_between_them():
    """k_assemble eliminates levels 1 and 2 unless level 2 is the top level (N < 3); cr_forward starts at level 4, whose U
    tasks are deferred to level 8 when there is one."""
    for N in LENGTHS:
        top, M = shim.top(N), N + 1
        fuse2 = N >= 3
        assert fuse2 == (top > 2)
        h0 = 4 if fuse2 else 2
        assert h0 <= top
        eliminated = {v for v in range(1, M + 1) if (v % 4 if fuse2 else v % 2)}
        touched = set()                                      # multiples of 4 that have absorbed what k_assemble left pending
        defer4 = h0 == 4 and top >= 8
        h = h0
        while h <= top:
            tasks, (countE, countU) = shim.level(N, h, updates=not (defer4 and h == 4))
            first = h0 == 4 and (h == 4 or (defer4 and h == 8))
            for kind, v in tasks:
                if h0 == 4:
                    assert (v not in touched) == first, (N, h, v)
                    touched.add(v)
                if first:
                    assert v % 4 == 0 and v // 4 - 1 >= 0    # pend[v / 4 - 1] exists
                if kind == "E":
                    eliminated.add(v)
            h <<= 1
        assert eliminated == set(range(1, M + 1)), N


def test_assemble_groups_cover_every_state_once():
    """k_assemble: group q holds the tree blocks 4q .. 4q+3 = states 4q-1 .. 4q+2; wavefront 0 of group 0 has no block"""
    for N in LENGTHS:
        M, groups = N + 1, shim.groups(N, 4)
        states, pend, coup = [], set(), set()
        for q in range(groups):
            live = [v for v in range(4 * q, 4 * q + 4) if 1 <= v <= M]
            assert live, (N, q)                              # no group is empty
            states += [v - 1 for v in live]
            if 4 * q + 4 <= M:
                pend.add(q)
                if q >= 1 and 4 * q + 2 <= M:
                    coup.add(q)
        assert states == list(range(N + 1)), N
        # level 4 finds what it asks for: pend[v/4 - 1] for every multiple of 4, coup for the pairs (v - 4, v), (v, v + 4)
        for v in range(4, M + 1, 4):
            assert v // 4 - 1 in pend
            if (v // 4) % 2 == 1:
                if v - 4 >= 1:
                    assert v // 4 - 1 in coup
                if v + 4 <= M:
                    assert v // 4 in coup
        assert max(pend | coup, default=0) < groups


def test_finish_groups_of_eight_cover_every_state_once():
    """k_finish_step / k_finish_trial: groups of 8 tree blocks 8q .. 8q+7; the multiples of 8 come from the solve kernel
    (levels >= 8), block 8q+4 needs x_{8q}, x_{8q+8}, then 8q+2 / 8q+6, then the odd ones -- the neighbours always sit in
    slots 0..8"""
    for N in range(16, 261):
        M, groups = N + 1, shim.groups(N, 8)
        handed = {8 * (k + 1) for k in range(M // 8)}        # what the step kernels copy to xg
        assert handed == set(range(8, M + 1, 8))
        seen = []
        for q in range(groups):
            have = {v for v in (8 * q, 8 * q + 8) if v in handed}
            for h, waves in ((4, (4,)), (2, (2, 6)), (1, (1, 3, 5, 7))):
                new = set()
                for wv in waves:
                    v = 8 * q + wv
                    if v > M:
                        continue
                    assert (v & -v) == h
                    for vn in (v - h, v + h):
                        if 1 <= vn <= M:
                            assert vn in have and 0 <= vn - 8 * q <= 8, (N, q, v, vn)
                    new.add(v)
                have |= new
            seen += sorted(v - 1 for v in have if v // 8 == q)
        assert seen == list(range(N + 1)), N


def test_fused_finish_windows_cover_every_state_once():
    """k_linearize_arm: the chunk of 64 evaluation points reads the states s0 .. s1 (<= ZNS) and owns those whose unary
    point lies in it; the window of FXS tree indices from the multiple of 8 below holds every block it must solve"""
    ZNS, FXS = shim.zns(), shim.fxs()
    assert (ZNS, FXS) == (24, 40)
    assert shim.chunk_states(2) <= ZNS < shim.chunk_states(1)        # the four-wavefront form needs obs_check_inter >= 2
    for I in (2, 3, 5, 10):
        for N in list(range(16, 131)) + [255, 256, 260]:
            M, P = N + 1, 1 + N * (I + 1)
            state_of = lambda pt: 0 if pt == 0 else 1 + (pt - 1) // (I + 1)
            owned = []
            for chunk in range((P + 63) // 64):
                p_lo, p_hi = chunk * 64, min(chunk * 64 + 63, P - 1)
                s1, s0 = state_of(p_hi), max(0, state_of(p_lo) - 1)
                assert s1 - s0 + 1 <= min(ZNS, shim.chunk_states(I))
                w0, need = shim.window(N, s0, s1)
                assert w0 % 8 == 0 and w0 <= s0 + 1
                have = set(need[8])
                assert all(v % 8 == 0 and 8 <= v <= M for v in have)
                for h in (4, 2, 1):
                    assert all((v & -v) == h and 1 <= v <= M and 0 <= v - w0 < FXS for v in need[h]), (N, I, chunk)
                    for v in need[h]:
                        for vn in (v - h, v + h):
                            if 1 <= vn <= M:
                                assert vn in have and 0 <= vn - w0 < FXS, (N, I, chunk, v, vn)
                    have |= need[h]
                assert set(range(s0 + 1, s1 + 2)) <= have, (N, I, chunk)
                owned += [s for s in range(s0, s1 + 1) if p_lo <= s * (I + 1) <= p_lo + 63]
            assert owned == list(range(N + 1)), (N, I)
