"""The block switching cases of switch_cases.py against the CPU oracle: the builder's own model of the output is the oracle's output,
the oracle counts the switches the builder counted, and the census of what the cases reach is complete.  No GPU."""
import functools
import warnings

import pytest

import oracle_py as oracle
import switch_cases


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = {c.name: c for c in switch_cases.all_cases()}[name]
    return oracle.decode(c.stream, 0, cap=len(c.out) + 64, want_stats=True)


def _names(valid):
    return [c.name for c in switch_cases.all_cases() if c.valid == valid]


def test_block_count_table_matches_the_anchors_of_the_format():
    """RFC 7932 section 6: code 0 = 1 + 2 bits, 16 = 241 + 6, 18 = 369 + 7, 25 = 16625 + 24; every range starts where the one before ends."""
    B = switch_cases.BLEN
    assert len(B) == 26
    assert (B[0], B[16], B[18], B[25]) == ((1, 2), (241, 6), (369, 7), (16625, 24))
    for k in range(25):
        assert B[k + 1][0] == B[k][0] + (1 << B[k][1]), k


@pytest.mark.parametrize("name", _names(True))
def test_valid_case_is_the_builders_output(name):
    c = {c.name: c for c in switch_cases.all_cases()}[name]
    st, out, stats = _oracle(name)
    assert st == 0 and len(out) == len(c.out)
    assert out == c.out, next(i for i, (a, b) in enumerate(zip(out, c.out)) if a != b)
    assert stats["block_switches"] == sum(c.switches), (stats["block_switches"], c.switches)
    assert stats["max_block_types"] == c.max_types


@pytest.mark.parametrize("name", _names(False))
def test_invalid_case_fails_behind_a_prefix_of_the_model(name):
    c = {c.name: c for c in switch_cases.all_cases()}[name]
    st, out, _ = _oracle(name)
    assert st not in (0, oracle.STATUS_OUTPUT_TOO_SMALL)
    assert c.out[:len(out)] == out


def test_truncations_fail_behind_a_prefix_of_the_model():
    cuts = switch_cases.truncations()
    assert 1500 <= len(cuts) <= 3000 and {n for n, _, _ in cuts} == set(switch_cases.TRUNCATED)
    for name, s, full in cuts:
        st, out = oracle.decode(s, 0, cap=len(full) + 64)
        assert st not in (0, oracle.STATUS_OUTPUT_TOO_SMALL) and full[:len(out)] == out, (name, len(s), st, len(out))


def test_the_case_list_is_what_the_issue_names():
    cases = switch_cases.all_cases()
    small = [c for c in cases if c.kind == "small"]
    assert all(400 <= len(c.stream) <= 4096 for c in small), [(c.name, len(c.stream)) for c in small]
    assert {c.max_types for c in small} >= {2, 3, 5, 16, 256}
    for k, cat in enumerate("LID"):
        assert any(c.name == "small_256_types_" + cat and c.switches[k] > 20 for c in small)
    assert all(min(c.switches) > 0 for c in cases if c.valid and c.kind != "top_bit"), "every valid case switches in all three categories"
    top = {c.name: c for c in cases}["top_bit"]
    assert len(top.out) > 16625 + (1 << 23) + 5 + 40000 and len(top.stream) > 5000
    assert sum(1 for c in cases if not c.valid) == 9


def test_census_is_complete_and_here_it_is():
    """Every key of the census has been reached (all_cases() asserts it as well).  The census is the assertion's message, and a
    passing run shows it as this test's one warning (pytest's warnings summary), so a reader sees what the cases reach."""
    census = switch_cases.census()
    keys = switch_cases.census_keys()
    assert len(keys) == len(set(keys))
    missing = [k for k in keys if not census.get(k)]
    lines = switch_cases.census_lines()
    warnings.warn("the census of the block switching cases (%d keys required, %d counted)\n%s" % (len(keys), len(census), "\n".join(lines)))
    assert not missing, "\n".join(["missing: %r" % (missing,)] + lines)
