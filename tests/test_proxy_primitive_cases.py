"""The case table of the proxy-side matrix (proxy_primitive_cases) is non-vacuous: a bad row fails
here, on a machine without a GPU, and not in the one program run on the GPU box."""
import os

import numpy as np
import pytest

import oracle_lib as O
import proxy_primitive_cases as C

T = [c for c in C.CASES if c.group == "T"]
F = [c for c in C.CASES if c.group == "F"]
P = [c for c in C.CASES if c.group == "P"]
R = [c for c in C.CASES if c.group == "R"]


def test_every_member_and_overload_appears():
    for op in C.PUT_FORMS:
        for bound in (0, 1):
            assert any(c.op == op and C.member(c).bound == bound for c in T), (op, bound)
            assert any(c.op == op and C.member(c).bound == bound for c in F), (op, bound)
            assert any(c.op == "place" and C.PUT_FORMS[c.v[1]] == op and c.v[0] == bound for c in P), (op, bound)
    for op in ("signal", "flush"):
        assert {C.member(c).bound for c in T if c.op == op} == {0, 1}
    assert {C.member(c).type for c in T if c.op == "push"} == set(range(1, 8))
    assert {c.op for c in F} >= {"push", "poll"}
    assert {c.op for c in P} == {"place", "order", "account", "laps"} and {c.op for c in R} == {"refuse"}
    assert set(C.MEMBER_OPS + C.PROXY_OPS) == {c.op for c in C.CASES}


# (fst mask, snd mask) of each field; the common-offset overloads put their offset into both offsets
FIELD_MASKS = dict(dstOff=(0, 0xFFFFFFFF), srcOff=(0xFFFFFFFF << 32, 0), size=(0xFFFFFFFF, 0), srcId=(0, 0x1FF << 32),
                   dstId=(0, 0x1FF << 41), semId=(0, 0x3FF << 53))


@pytest.mark.parametrize("op", C.PUT_FORMS + ["push"])
def test_every_field_takes_each_extreme_and_it_changes_the_image(op):
    """Alone and all at once; and against the same case with the default in that field, the expected
    slot differs in exactly that field's bits."""
    rows = [c for c in T if c.op == op and C.expected_member(c)["err0"] == 0]
    for bound in ((0, 1) if op != "push" else (0,)):
        mine = [c for c in rows if C.member(c).bound == bound]
        base_type = 5 if op == "push" else 0
        default = next(c for c in mine if c.tag.endswith("defaults") and C.member(c).type in (base_type, 1))
        for field, values in C.FIELD_VALUES.items():
            if op.endswith("_same") and field == "srcOff":
                continue
            for x in values:
                alone = [c for c in mine if getattr(C.member(c), field) == x and
                         all(getattr(C.member(c), g) == C.DEFAULTS[g] for g in C.FIELD_VALUES if g != field)]
                assert alone, (op, bound, field, x)
                together = [c for c in mine if getattr(C.member(c), field) == x and
                            all(getattr(C.member(c), g) != C.DEFAULTS[g] for g in C.FIELD_VALUES)]
                assert together, (op, bound, field, x, "all at once")
                c = alone[0]
                d = default._replace(v=C.member(default)._replace(type=C.member(c).type))
                a, b = C.expected_member(c)["ring"][0], C.expected_member(d)["ring"][0]
                diff = int(a[0]) ^ int(b[0]), int(a[1]) ^ int(b[1])
                mask = FIELD_MASKS[field]
                if op.endswith("_same") and field == "dstOff":
                    mask = (FIELD_MASKS["srcOff"][0], mask[1])
                assert diff != (0, 0) and diff[0] & ~mask[0] == 0 and diff[1] & ~mask[1] == 0, C.describe(c)


def test_a_swap_changes_the_image():
    """dstId != srcId and dstOffset != srcOffset wherever a case has both; the common-offset
    overloads are the rows that say otherwise."""
    for c in T + F:
        if c.op not in C.PUT_FORMS + ["push"]:
            continue
        h = C.member(c)
        assert h.dstId != h.srcId, C.describe(c)
        for i in range(h.active * h.count):
            t = C.call_trigger(c, i)
            if t is None:
                continue
            if c.op.endswith("_same"):
                assert t[2] == t[4]
            else:
                assert t[2] != t[4], C.describe(c)
                swapped = (t[0], t[3], t[4], t[1], t[2], t[5], t[6])
                assert C.encode(*swapped) != C.encode(*t)
    for c in P + R:
        for dst_id, dst_off, src_id, src_off, size in C.puts_of(c)[0] + ([tuple(c.v[:5])] if c.op == "refuse" else []):
            same_form = c.op == "place" and C.PUT_FORMS[c.v[1]].endswith("_same")
            assert (dst_off == src_off) == same_form, C.describe(c)
            assert dst_id != src_id or c.tag.startswith("same-id"), C.describe(c)
    assert sum(c.tag.startswith("same-id") for c in P) == C.N_MEM


def test_too_wide_values_go_through_every_put_form():
    for op in C.PUT_FORMS:
        for bound in (0, 1):
            fields = ("dstOff", "size") if op.endswith("_same") else ("dstOff", "srcOff", "size")
            for field in fields:
                rows = [c for c in T if c.op == op and C.member(c).bound == bound and getattr(C.member(c), field) == 1 << 32]
                assert len(rows) == 1 and not rows[0].ref
                e = C.expected_member(rows[0])
                assert e["err0"] == C.ERR_BAD_GEOMETRY and e["head"] == 0 and not e["ring"].any()
    # and nothing else is kept from the reference build in groups T and F
    assert all(c.ref == (C.expected_member(c)["err0"] == 0) for c in T + F)
    assert not any(c.ref for c in P + R)


def test_group_f_laps_and_shapes():
    for ring, r in C.SEQ_RINGS.items():
        assert 0 < r < ring
        counts = sorted(C.member(c).count for c in F if c.tag.startswith(f"seq-ring{ring}-"))
        assert counts == [k * ring + r for k in range(4)]
        third = next(c for c in F if c.tag.startswith(f"seq-ring{ring}-k2"))
        e = C.expected_member(third)
        assert e["head"] == 2 * ring + r and e["tailCache"] == e["tail"] == e["head"]
        # the last lap is partial: its first r slots carry lap 2's commit bit (1), the others lap 1's (0)
        commit = [int(s) >> 63 for s in e["ring"][:, 1]]
        assert commit == [1] * r + [0] * (ring - r)
        assert [int(s) & 0xFFFFFFFF for s in e["ring"][:, 1]] == [2 * ring + i for i in range(r)] + \
            [ring + i for i in range(r, ring)]
    shapes = [(C.member(c).grid, C.member(c).lanes, C.member(c).active) for c in F if c.op == "push" and
              c.tag.startswith("lanes-")]
    assert shapes == C.LANE_SHAPES and [s[2] for s in shapes] == [1, 63, 64, 65, 256]
    for c in F:
        h = C.member(c)
        assert h.active <= h.grid * h.lanes
        if h.active > 1:
            assert h.active * h.count <= h.ring, "concurrent pushers must not exceed the FIFO size"
        if h.active * h.count > h.ring:
            assert h.tail == h.active * h.count
    polls = {C.member(c).dstOff - C.member(c).tail: C.expected_member(c) for c in F if c.op == "poll"}
    assert sorted(polls) == [-1, 0, 1]
    assert polls[-1]["pos"] == [1] and polls[-1]["tailCache"] == 5
    assert polls[0]["pos"] == [0] and polls[1]["pos"] == [0] and polls[0]["tailCache"] == 0


def test_no_member_case_can_wait():
    """The program refuses these too; a bad row fails here first."""
    for c in T + F:
        h = C.member(c)
        if c.op in C.FLUSH_OPS:
            assert h.flushDone > h.active * h.count
        C.expected_member(c)  # replay asserts that no sync would have to wait


def test_group_p_rows_stay_inside_and_destinations_are_disjoint():
    pairs, pairings, sizes = set(), set(), set()
    for c in P:
        puts = C.puts_of(c)[0]
        spl = C.splits(c)
        taken = []
        for dst_id, dst_off, src_id, src_off, size in puts:
            assert dst_id < C.N_MEM and src_id < C.N_MEM
            assert dst_off + size <= C.ARENA and src_off + size <= C.ARENA, C.describe(c)
            assert src_off + size <= spl[src_id] or size == 0, "a source range lies in seeded bytes"
            assert dst_off >= spl[dst_id], "a destination range lies in 0xA5 bytes"
            for a, lo, hi in taken:
                assert a != dst_id or dst_off + size <= lo or hi <= dst_off, C.describe(c)
            taken.append((dst_id, dst_off, dst_off + size))
            if c.op == "place":
                if not c.v[0]:
                    pairs.add((dst_id, src_id))
                else:
                    assert (dst_id, src_id) == (C.BOUND_DST, C.BOUND_SRC)
                if not c.tag.startswith("same-id"):
                    pairings.add((dst_off % 16, src_off % 16))
                    sizes.add(size)
    assert pairs == {(d, s) for d in range(C.N_MEM) for s in range(C.N_MEM)}
    assert pairings == {(d, s) for d in C.ALIGN_OFFSETS for s in C.ALIGN_OFFSETS}
    assert sizes == {0, 1, 15, 16, 17, 4099, (64 << 10) + 19}
    for c in P:
        if c.op == "place" and not c.tag.startswith("same-id"):
            assert sorted(p[4] for p in C.puts_of(c)[0]) == sorted(C.PLACE_SIZES)
    assert sorted(c.v[0] for c in P if c.op == "order") == [16, 4099, (64 << 10) + 19]
    assert all(c.v[1] == 3 and c.v[4] > 0 for c in P if c.op == "order")
    assert sorted({c.v[0] for c in P if c.op == "account"}) == [1, 3, 9]
    assert all(c.v[1] <= c.v[0] for c in P if c.op == "account")
    assert sorted(C.puts_of(c)[1] for c in P if c.op == "laps") == [8 + 8, 43 + 1, 48 + 1]
    assert C.PROXY_FIFO == 8


def test_group_r_rows_cross_exactly_one_bound_by_one():
    kinds = set()
    for c in R:
        dst_id, dst_off, src_id, src_off, size = c.v[:5]
        crossed = []
        if dst_id >= C.N_MEM:
            crossed.append(("dst id", dst_id - (C.N_MEM - 1)))
        if src_id >= C.N_MEM:
            crossed.append(("src id", src_id - (C.N_MEM - 1)))
        if dst_off + size > C.ARENA:
            crossed.append(("dst range", dst_off + size - C.ARENA))
        if src_off + size > C.ARENA:
            crossed.append(("src range", src_off + size - C.ARENA))
        assert len(crossed) == 1 and crossed[0][1] == 1, C.describe(c)
        kinds.add(crossed[0][0])
        assert C.fits(C.T_DATA, dst_id, dst_off, src_id, src_off, size, 0), "the refused put must reach the proxy"
        (g_dst, g_off, g_src, g_soff, g_size), pushed, _ = C.puts_of(c)[0][0], *C.puts_of(c)[1:]
        assert pushed == 3 and g_off + g_size <= C.ARENA and g_soff + g_size <= C.ARENA
        if dst_id < C.N_MEM:  # the valid put goes to another cell
            assert g_dst != dst_id or g_off + g_size <= dst_off or dst_off + size <= g_off
    assert kinds == {"dst id", "src id", "dst range", "src range"}


def _tuples():
    seen = set()
    for c in T + F:
        h = C.member(c)
        for i in range(h.active * h.count):
            t = C.call_trigger(c, i)
            if t is not None:
                seen.add(t)
    return sorted(seen)


def test_model_encoding_agrees_with_both_restatements():
    tuples = _tuples()
    assert len(tuples) > 300
    for t in tuples:
        assert C.encode(*t) == O.trigger_encode(*t), t
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v1.npz"))
    rows = [[int(x) for x in row] for row in g["triggers"]]
    assert rows
    for *t, fst, snd in rows:
        assert C.fits(*t) and C.encode(*t) == (fst, snd), t
    # the commit bit is bit 63 of snd and nothing else
    t = tuples[-1]
    assert C.encode(*t, commit=1) == (C.encode(*t)[0], C.encode(*t)[1] | 1 << 63)


def test_case_file_round_trip(tmp_path):
    path = str(tmp_path / "cases.txt")
    C.write_case_file(path)
    assert C.parse_case_file(path) == [(c.idx, c.op, c.v) for c in C.CASES]
    C.write_case_file(path, for_reference=True)
    assert C.parse_case_file(path) == [(c.idx, c.op, c.v) for c in C.CASES if c.ref]
    assert [c.idx for c in C.CASES] == list(range(len(C.CASES)))
    assert all(len(c.v) <= 48 for c in C.CASES)
