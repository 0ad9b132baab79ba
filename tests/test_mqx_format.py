"""CPU: tests/mqx.py against itself and against the oracle -- the second implementation of the index file, the model of the
probe order, and the preconditions of the crafted tables that tests/test_gpu_crafted_tables.py loads on the GPU (a table must
force what its row claims: computed here from the oracle's keys and `probe_order` alone, for fixed seeds)."""
import numpy as np
import pytest

import mqx

LEG_NAMES = ("small", "default")


def all_tables(src, leg):
    """every crafted table of a leg (the default leg carries the tables whose cost grows with the key count only once)"""
    ts = [mqx.rehoused(src), mqx.rehoused(src, 4), mqx.one_empty(src), mqx.key0(src, "live"), mqx.key0(src, "dead"), mqx.key0(src, "absent")]
    if leg == "small":
        ts += [mqx.table_end(src), mqx.dead(src), mqx.ids(src)] + mqx.tiny_tables(src)
    return ts


@pytest.fixture(scope="module", params=LEG_NAMES)
def leg(request, oracle, simlib):
    return request.param, mqx.source(oracle, simlib, request.param)


def test_roundtrip_and_header_rule(leg, oracle, tmp_path):
    """write -> read gives the same parameters, header, references and slots for every crafted table, and the header's
    n_keys / n_unique (the reference's rule, src/index.rs:67-69, 90-104) are what the oracle's map counts after the same
    insertions."""
    name, src = leg
    for i, t in enumerate(all_tables(src, name)):
        p = str(tmp_path / ("t%d.mqx" % i))
        hdr = t.to_file(p)
        pr, hr, refs, slots = mqx.read(p)
        assert pr == t.params and hr == hdr == t.header() and refs == t.refs, t.name
        assert slots.tobytes() == t.slots().tobytes(), t.name
        assert hr["n_keys"] == t.entries.size < t.table_slots, t.name
        ox = t.to_oracle(oracle)
        assert (ox.keys(), ox.count()) == (hr["n_keys"], hr["n_unique"]), t.name
        assert hr["n_unique"] == int(t.live_mask().sum()), t.name
        for rid, rname, rlen in t.refs:
            assert (ox.ref_name(rid), ox.ref_len(rid)) == (rname, rlen), t.name


def test_source_entries_are_the_oracles_index(leg, oracle):
    """The key set a crafted table is made of IS the genome's index: `rehoused` through `add` answers every key like the
    oracle's own index built from the sequences."""
    name, src = leg
    ox, twin = src.oracle_index(oracle), mqx.rehoused(src).to_oracle(oracle)
    assert (ox.keys(), ox.count()) == (twin.keys(), twin.count()) == (src.entries.size, int((src.entries["count"] == 1).sum()))
    for h in np.concatenate([src.entries["key"][::7], src.read_keys[::5]]):
        a, b = ox.get(int(h)), twin.get(int(h))
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())


def test_header_rule_small_cases():
    s = np.zeros(6, dtype=mqx.slot_dtype)
    s["key"] = [9, 10, 11, 12, 0, 13]
    s["count"] = [1, 2, 0xFFFFFFFF, 1, 1, 1]
    s["end"] = [5, 5, 5, 0, 5, 5]
    assert mqx.header_counts(s) == (6 + 0xFFFFFFFF, 6, 3)
    s["key"][5] = 9  # the same key in two slots: inserted twice
    assert mqx.header_counts(s)[1:] == (5, 1)
    assert mqx.header_counts(s[:0]) == (0, 0, 0)


@pytest.mark.parametrize("ts", [2, 4, 8, 1024])
def test_probe_order_visits_every_slot_once(ts):
    rng = np.random.default_rng(ts)
    keys = [1, 2, 3, ts - 1, ts, ts + 1, 2**64 - 1, 2**64 - 2] + [int(x) for x in rng.integers(1, 2**64, size=40, dtype=np.uint64)]
    for k in keys:
        o = mqx.probe_order(k, ts)
        assert sorted(o) == list(range(ts)), (k, ts)
        assert o[0] == k & (ts - 1) and o[1] == o[0] ^ 1
        nb = ts // 2
        for j in range(1, nb):  # bucket after bucket, way 0 first, wrapping behind the last bucket
            b = ((o[0] >> 1) + j) % nb
            assert o[2 * j:2 * j + 2] == [2 * b, 2 * b + 1]
    assert mqx.probe_order(0, ts) == [ts]


def test_preconditions_of_the_plans(leg, oracle):
    """Section by section what each table's row claims, from the oracle's keys and the probe order alone."""
    name, src = leg
    po = src.po
    b, o = src.reads["bases"], src.reads["offsets"]
    built = src.oracle_index(oracle).map_batch(b, o, po, threads=4)
    assert mqx.n_mapped(built) >= 0.5 * (o.size - 1)
    small = mqx.rehoused(src)
    mqx.check_rehoused(small)
    oe = mqx.one_empty(src)
    mqx.check_one_empty(oe, src)
    # the full-key-set tables are the same map: at least 90 % of the reads the built index maps stay mapped (all of them do)
    for t in (small, oe, mqx.key0(src, "live")):
        w = t.to_oracle(oracle).map_batch(b, o, po, threads=4)
        still = int(((w["mapped"] != 0) & (built["mapped"] != 0)).sum())
        assert still >= 0.9 * mqx.n_mapped(built), t.name
        assert w.tobytes() == built.tobytes(), t.name
    # what probe_stats is held against on the GPU: both bounds say something (thousands of certain steps)
    assert mqx.miss_lookups(oe, src).size - mqx.max_misses_at_one_slot(oe, src) >= 900 and mqx.certain_steps(small, src) >= 100
    if name == "small":
        te = mqx.table_end(src)
        mqx.check_table_end(te, src)
        w = te.to_oracle(oracle).map_batch(b, o, po, threads=4)
        assert mqx.n_mapped(w) >= 20
        d = mqx.dead(src)
        assert d.changed.size >= 40 and d.header()["n_unique"] == small.header()["n_unique"] - d.changed.size
        tiny = mqx.tiny_tables(src)
        assert [(t.table_slots, t.entries.size) for t in tiny] == [(s, n) for s in (2, 4, 8) for n in range(1, s)]
