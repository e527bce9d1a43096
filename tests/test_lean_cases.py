"""tests/lean_cases.py pinned on the CPU oracle: the plain set is valid and reaches every feature it is named after (read off the
oracle's census), the deferred set holds a named case for every way out of the lean kernel, and both lookup modes of the oracle
agree on all of it.  No GPU."""
import os
import re

import lean_cases as lc
import oracle_py as oracle

ROOT_SMALL_H = os.path.join(oracle.ROOT, "brotli-rs_amd", "csrc", "brx_small.h")


# text of a `return SM_DEFER` line of brx_small.h, how often it occurs, the cases that take it (prefixes of case names)
SITES = [
    ("hb_bits(d, 3) != 0u", 1, ["two_literal_block_types", "two_distance_block_types", "block_type_incomplete_code"]),
    ("rlemax + t.ntl, h)", 1, ["bad_literal_map_code"]),
    ("t.cml, 64u)", 1, ["bad_literal_map_body", "incomplete_code_context_map"]),
    ("rlemax + t.ntd, h)", 1, ["bad_distance_map_code"]),
    ("t.cmd, 4u)", 1, ["bad_distance_map_body"]),
    ("if (d.scr_top) return", 1, ["tree_handles_beyond_table_memory"]),
    ("alphabet, h, i > t.ntl)", 1, ["bad_literal_tree", "forty_literal_trees_"]),
    ("(hv_), lit)", 1, ["incomplete_code_literal"]),
    ("if (hb_over(d)) return", 2, ["prefix_"]),  # a cut inside the commands / inside a meta-block header
    ("h_i, hv_i, sym)", 1, ["incomplete_code_iac"]),
    ("insert_len > mb_left", 1, ["insert_past_mlen"]),
    ("h_d0, hv_d0, dcode)", 1, ["incomplete_code_distance"]),
    ("h, hv, dcode)", 1, ["distance_tree_of_context_incomplete"]),
    ("basev <= delta", 1, ["non_positive_distance"]),
    ("ndistbits > 24u", 1, None),  # unreachable: a distance symbol is below 48 << NPOSTFIX behind the direct ones, so ndistbits <= 24
    ("copy_len > mb_left", 1, ["copy_past_mlen"]),
    ("copy_len < 4u || copy_len > 24u", 1, ["dictionary_length_3", "dictionary_length_25"]),
    ("dict_word(", 1, ["transform_id_121", "dictionary_reference_panics"]),
    ("wl > mb_left", 1, ["dictionary_word_past_mlen"]),
    ("if (v == 1u) return", 1, ["reserved_wbits"]),
    ("nib == 3u", 1, ["metadata_block"]),
    ("mnibbles > 4u && (v >>", 1, ["trailer_nibble_5", "trailer_nibble_6"]),
    ("(u64)d.pos + mlen > (u64)d.cap", 1, ["capacity_"]),
    ("if (k && hb_bits(d, 8u - k) != 0u) return", 2, ["raw_non_zero_fill_bits", "trailing_bit_"]),
    ("p + 8ull * mlen > d.bitend", 1, ["raw_longer_than_input"]),
    ("if (sm_header(d, s, t)) return", 1, ["bad_literal_tree"]),      # (passes the header's own exits on)
    ("if (sm_commands(", 1, ["insert_past_mlen"]),                    # (passes the command loop's own exits on)
    ("hb_pos(d) != d.bitend", 1, ["appended_00_", "appended_01_"]),
]  # (and the kernel itself lists a stream of no bytes at all: empty_input)


def _census(cases):
    """The census fields of the cases' streams, OR-ed (masks) / summed (counters are only tested against 0) / as sets (wbits)."""
    agg = {}
    for c in cases:
        for k, v in lc.full(c.data)[2].items():
            if k == "wbits":
                agg.setdefault(k, set()).add(v)
            elif k.startswith("max_"):
                agg[k] = max(agg.get(k, 0), v)
            else:
                agg[k] = agg.get(k, 0) | v if k.endswith(("_mask", "_lo", "_hi", "_trees", "single_codes")) else agg.get(k, 0) + v
    return agg


def test_every_plain_case_is_valid_and_owned_by_the_lean_kernel():
    P = lc.plain_set()
    assert len({c.name for c in P}) == len(P)
    for c in P:
        st, out, census = lc.full(c.data)
        assert st == 0 and c.status == 0 and c.out == out and c.out_len == len(out), c.name
        assert c.cap % 2 == 1 and c.cap >= len(out), c.name
        assert census["max_table_words"] <= 400, (c.name, census["max_table_words"])  # well inside the 512 words
        assert census["metadata_blocks"] == 0 and census["max_block_types"] <= 1, c.name
        assert c.owner == ("lean" if len(c.data) <= lc.SMALL_MAX else "regular"), c.name
    assert [c.name for c in P if c.owner == "regular"] == ["edge_501_eight_trees"]
    assert sum(128 < len(c.data) <= 500 for c in P) >= 40


def test_size_edges():
    sizes = {len(c.data) for c in lc.plain_set() if "edge" in c.tags}
    assert sizes == set(lc.SIZE_EDGES) | {501}
    assert lc.plain_set()[0].data == b"\x06"
    # in the batch the GPU tests decode, every edge case starts at each of the four input phases, behind junk streams that are cases of
    # their own
    slots = lc.full_batch()
    for c in slots:
        if "junk" in c.tags:
            assert 1 <= len(c.data) <= 3 and (c.status == 0) == (c.data == b"\x06") and c.owner == ("lean" if c.status == 0 else "regular")
    phases = lc.phases(slots)
    assert all(p == {0, 1, 2, 3} for p in phases.values()) and len(phases) == len([c for c in lc.plain_set() if "edge" in c.tags])
    assert {c.name for c in slots} >= {c.name for c in lc.plain_set() + lc.deferred_set()}


def test_plain_set_reaches_every_feature():
    P = [c for c in lc.plain_set() if c.owner == "lean"]
    a = _census(P)
    by = {c.name: lc.full(c.data)[2] for c in P}
    # header shapes
    assert a["wbits"] == set(range(10, 25))
    assert a["mnibbles_mask"] == (1 << 4) | (1 << 5) | (1 << 6)
    for np_ in range(4):
        assert [by[n]["ndirect_mask"] for n in by if n.startswith("npostfix_%d_" % np_)] == [1, 2]
        assert all(by[n]["npostfix_mask"] == 1 << np_ for n in by if n.startswith("npostfix_%d_" % np_))
    assert by["two_meta_blocks"]["meta_blocks"] == 2 and by["two_meta_blocks"]["raw_blocks"] == 0
    assert by["two_meta_blocks_empty_last"]["empty_last"] == 1 and a["empty_last"] >= 3
    for n in (1, 63, 64, 65):
        f, m = by["raw_%d_in_front" % n], by["raw_%d_between" % n]
        assert f["raw_bytes"] == n and f["meta_blocks"] == 2 and m["raw_bytes"] == n and m["meta_blocks"] == 3
    assert by["raw_only"]["commands"] == 0
    # trees
    for mode in range(4):
        for ntl in (1, 2, 3, 4, 8):
            assert a["ntrees_l_mask"] >> (16 * mode + ntl) & 1, (mode, ntl)
    assert a["ntrees_d_mask"] & 0b10110 == 0b10110
    four = [v for n, v in by.items() if "_ntd4_" in n]
    assert four and all(v["dist_ctx_trees"] == 0x8421 for v in four)  # context k reads tree k, all four of them
    assert a["cmap_rle"] >= 4 and a["cmap_imtf"] >= 4
    assert by["one_symbol_codes"]["single_codes"] == 7
    # commands
    assert by["one_symbol_insert_24_extra_bits"]["max_insert_extra"] == 24 and by["copy_lengths_2_33"]["max_insert_extra"] >= 5
    assert any(v["commands"] and v["max_insert_extra"] == 0 for v in by.values())
    assert a["copy_len_lo"] == (1 << 64) - 4  # every copy length 2..63
    longer = by["copy_lengths_65_70_1000"]
    assert by["copy_lengths_34_64"]["max_copy_len"] == 64 and longer["max_copy_len"] >= 60000 and longer["copy_bytes"] < 65536
    assert a["short_dist_mask"] & 0b1110 == 0b1110 and a["overlapped_copies"] and a["dist_eq_len"] and a["dist_gt_len"] and a["dist_at_max"]
    assert by["far_copies"]["max_distance"] > lc.RING_BYTES
    assert any(by["wbits_%d" % w]["max_distance"] == (1 << w) - 16 for w in (10, 11))  # exactly the window
    ring = _census([c for c in P if c.name.startswith("ring_codes")])
    assert ring["dist_code_mask"] == (1 << 18) - 1 and ring["implicit_dist0"] >= 10
    d = _census([c for c in P if "dictionary" in c.tags])
    assert d["xform_lo"] == (1 << 64) - 1 and d["xform_hi"] == (1 << 57) - 1 and d["dict_len_mask"] == (1 << 25) - (1 << 4)
    red = [c for c in P if "alphabet" in c.tags]
    assert len(red) >= 10 and sum(len(c.data) > 128 for c in red) >= 5


def test_every_way_out_of_the_lean_kernel_has_a_named_case():
    D = lc.deferred_named()
    assert len({c.name for c in D}) == len(D)
    for c in D:
        assert c.owner == ("lean" if "capacity" in c.tags and c.status == 0 else "regular"), c.name
        if "capacity" in c.tags:
            assert c.status in (0, 25) and (c.status == 25) == (c.cap < len(lc.full(c.data)[1])), c.name
    want = {"empty_input": 24, "reserved_wbits": 24, "trailer_nibble_5": 16, "trailer_nibble_6": 16, "raw_non_zero_fill_bits": 13,
            "raw_longer_than_input": 24, "insert_past_mlen": 3, "copy_past_mlen": 3, "dictionary_word_past_mlen": 3,
            "non_positive_distance": 10, "dictionary_length_3": 6, "dictionary_length_25": 6, "transform_id_121": 9,
            "dictionary_reference_panics": 26, "incomplete_code_literal": 21, "incomplete_code_iac": 20, "incomplete_code_distance": 19,
            "distance_tree_of_context_incomplete": 19, "incomplete_code_context_map": 17, "bad_literal_map_code": 8,
            "bad_literal_map_body": 17, "bad_distance_map_code": 8, "bad_distance_map_body": 17, "bad_literal_tree": 8,
            "block_type_incomplete_code": 5, "trailing_bit_edge_1": 15}
    by = {c.name: c for c in D}
    for name, st in want.items():
        assert by[name].status == st, (name, by[name].status)
    # valid streams that are not plain: the census says why
    for name in ("metadata_block", "metadata_block_skip"):
        assert by[name].status == 0 and lc.full(by[name].data)[2]["metadata_blocks"] == 1
    for name in ("two_literal_block_types", "two_distance_block_types"):
        assert by[name].status == 0 and lc.full(by[name].data)[2]["max_block_types"] == 2
    forty = [c for c in D if c.name.startswith("forty_literal_trees")]
    assert len(forty) == 3 and all(c.status == 0 and len(c.data) <= 500 and lc.full(c.data)[2]["max_table_words"] >= 600 for c in forty)
    assert lc.full(by["tree_handles_beyond_table_memory"].data)[2]["bits_consumed"] > 0
    for c in lc.base_streams():
        assert by["appended_00_" + c.name].status == 2 and by["appended_01_" + c.name].status == 2
        assert any(n.startswith("trailing_bit_") and n.endswith(c.name) and by[n].status == 15 for n in by) or \
            8 * len(c.data) == lc.full(c.data)[2]["bits_consumed"]
    assert sum("capacity" in c.tags for c in D) == 30
    # every `return SM_DEFER` of brx_small.h is one of SITES, as often as the table says, and its cases exist
    names = {c.name for c in lc.deferred_set()}
    lines = [ln.strip() for ln in open(ROOT_SMALL_H) if "return SM_DEFER" in ln]
    for ln in lines:
        assert sum(site in ln for site, _, _ in SITES) == 1, "a way out of the lean kernel without a case in SITES: " + ln
    for site, count, cases in SITES:
        assert sum(site in ln for ln in lines) == count, site
        assert cases is None or (cases and all(any(n.startswith(c) for n in names) for c in cases)), site


def test_stream_ends_and_bit_flips():
    sizes = sorted(len(c.data) for c in lc.base_streams())
    assert 120 <= sizes[0] <= 160 and sizes[1] == 258 and sizes[2] == 500
    pre = lc.prefix_set()
    assert len(pre) == sum(sizes) - 3 and all(c.status != 0 and c.owner == "regular" for c in pre)
    assert sum(c.status == 24 for c in pre) >= len(pre) - 6  # (a cut on a byte boundary in front of padding may end otherwise)
    flips = lc.bitflip_set()
    assert len(flips) == 8 * sum(sizes) >= 7000
    assert {c.status for c in flips} >= {0, 24}  # (MLEN bounds every item: no flip of these three streams outgrows 8 KiB -- 25 is the capacity cases')
    for c in flips:
        assert c.cap == lc.ERR_CAP and (c.owner == "lean") == (lc.owner_of(c.data, c.cap) == "lean")
        if c.owner == "lean":
            assert c.status == 0
    assert len({c.status for c in flips}) >= 8


def test_both_lookup_modes_agree():
    for c in lc.plain_set() + lc.deferred_named() + lc.prefix_set()[::7] + lc.bitflip_set()[::5]:
        assert oracle.decode_at(c.data, c.cap, oracle.FLAG_TREE_WALK) == (c.status, c.out_len, c.out), c.name


def test_the_builder_is_deterministic():
    def snap():
        return [(c.name, c.data, c.cap, c.status, c.out_len, c.owner) for c in lc.plain_set() + lc.deferred_named()] + \
               [(c.name, c.data) for c in lc.prefix_set()[::50] + lc.bitflip_set()[::50]]

    first = snap()
    for f in (lc.plain_set, lc.deferred_named, lc.prefix_set, lc.bitflip_set, lc.base_streams):
        f.cache_clear()
    assert snap() == first


def test_owner_follows_small_bytes():
    P = lc.plain_set()
    at128 = lc.with_small_bytes(P, 128)
    assert all((c.owner == "lean") == (len(c.data) <= 128) for c in at128)
    assert all(c.owner == "regular" for c in lc.with_small_bytes(P, 0))
