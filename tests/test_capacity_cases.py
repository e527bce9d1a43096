"""The case table of tests/capacity_cases.py, checked on the CPU: tests/test_gpu_capacity.py holds the kernels to it."""
import collections

import capacity_cases as cc
import oracle_py as oracle


def _by_stream():
    by = collections.defaultdict(list)
    for c in cc.table():
        by[c.stream].append(c)
    return by


def test_the_edges_the_fixtures_are_known_to_have():
    idx = {s.name: i for i, s in enumerate(cc.streams())}
    for name, cap, status, out_len in [("alice29.txt", 0, 25, 4), ("alice29.txt", 152088, 25, 152089), ("alice29.txt", 152089, 0, 152089),
                                       ("compressed_repeated", 0, 25, 50402), ("zeros", 1, 25, 262144), ("backward65536", 1, 25, 256)]:
        got = [c for c in cc.table() if c.stream == idx[name] and c.cap == cap]
        assert len(got) == 1 and (got[0].status, got[0].out_len) == (status, out_len), (name, cap, got)


def test_valid_streams_give_25_below_their_length_and_0_from_there_on():
    for si, cases in _by_stream().items():
        s = cc.streams()[si]
        if not s.valid:
            continue
        last = 0
        for c in cases:
            assert c.status in (0, 25), (s.name, c)
            assert (c.status == 25) == (c.cap < s.L), (s.name, c)
            if c.status == 25:
                assert c.cap < c.out_len <= s.L, (s.name, c)  # (needed: beyond the slot, never beyond the stream)
            else:
                assert c.out_len == s.L == c.n_bytes, (s.name, c)
            assert c.out_len >= last, (s.name, c)  # non-decreasing in the capacity
            last = c.out_len


def test_invalid_streams_give_25_in_front_of_the_error_and_the_error_behind_it():
    """Ordered in the capacity: status 25 with a non-decreasing `needed` up to some capacity, the stream's own error from there on,
    always at the same position.  An item that does not fit is refused in front of the error, never behind it."""
    for si, cases in _by_stream().items():
        s = cc.streams()[si]
        if s.valid:
            continue
        statuses = [c.status for c in cases]
        first_err = statuses.index(s.status)
        assert 0 < first_err and statuses == [25] * first_err + [s.status] * (len(cases) - first_err), (s.name, statuses)
        last = 0
        for c in cases[:first_err]:
            assert c.cap < c.out_len and c.out_len >= last, (s.name, c)
            last = c.out_len
        for c in cases[first_err:]:
            assert c.out_len == s.L and c.n_bytes == min(s.L, c.cap), (s.name, c)


def test_the_table_is_complete():
    by = _by_stream()
    names = [s.name for s in cc.streams()]
    assert len(set(names)) == len(names) == 21 and set(cc.FIXTURES) <= set(names)
    assert len(cc.table()) >= 1000, len(cc.table())
    assert len({(c.stream, c.cap) for c in cc.table()}) == len(cc.table())  # deduplicated
    for si, s in enumerate(cc.streams()):
        caps = {c.cap for c in by[si]}
        assert {0, 1, 15, 16, 17, s.L // 2, max(s.L - 1, 0), s.L, s.L + 1} <= caps, s.name
        assert all(c >= 0 for c in caps)
        short = [c for c in by[si] if c.status == 25 and c.out_len == c.cap + 1]  # one byte short of an item's end ...
        assert s.L == 0 or any(c.out_len in caps for c in short), s.name  # ... and the slot that just holds the item
        for e in s.ends:
            assert {e - 1, e, e + 1} <= caps, (s.name, e)
        if s.name != "empty":
            assert len({c.status for c in by[si]}) == 2, s.name
        else:
            assert [(c.status, c.out_len) for c in by[si]] == [(0, 0)] * len(by[si])
    multi = cc.streams()[names.index("four_meta_blocks")]
    assert len(multi.ends) >= 3 and multi.ends[-1] == multi.L and all(200 <= b - a <= 999 for a, b in zip((0,) + multi.ends, multi.ends))
    assert cc.streams()[names.index("raw_9000")].ends[0] >= 8192 > cc.streams()[names.index("raw_8000")].ends[0]


def test_guard_cases_cover_every_stream_and_both_statuses():
    g = cc.guard_cases()
    assert 150 <= len(g) <= 260, len(g)
    assert {c.stream for c in g} == set(range(len(cc.streams())))
    for si, s in enumerate(cc.streams()):
        mine = {c.cap: c for c in g if c.stream == si}
        assert {s.L + p for p in (0, 1, 7, 13)} | {0, 1, max(s.L - 1, 0)} <= set(mine), s.name
        if s.valid:
            assert all(mine[s.L + p].status == 0 for p in (0, 1, 7, 13)), s.name
            # one byte short of an item's end: status 25 and exactly that end
            assert s.L == 0 or any(c.status == 25 and c.out_len == c.cap + 1 for c in mine.values()), s.name


def test_tree_walk_mode_gives_the_same_table():
    assert cc.tree_walk_table() == cc.table()


def test_facade_retry_replay():
    """Which streams the Read facade's first guess holds.  (64x decodes to 64 bytes: it fits, with no retry.)"""
    for name in ("quickfox_repeated", "zeros", "backward65536"):
        data = cc.read(name + ".compressed")
        assert oracle.decode_at(data, (8 * len(data) + 65536 + 15) & ~15)[0] == 25, name
        assert cc.facade_retries(data) >= 1, name
    for name in ("alice29.txt", "monkey", "x", "64x"):
        assert cc.facade_retries(cc.read(name + ".compressed")) == 0, name
