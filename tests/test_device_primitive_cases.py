"""The tables of device_primitive_cases are not vacuous: every <Alignment, CopyRemainder> of every
Group A primitive meets a head, a tail, a size below the head, a ragged size and the lane shapes
that matter; the wrong models a test must tell from the right one (target and origin swapped, the
remainder flag flipped, the LL16 packet count rounded up, the reference's unclamped head) all differ
on the cases meant for them; the arenas keep their guard bands; the case file round-trips; and an
element-by-element restatement of copyHelper agrees with the sliced model on the whole table."""
import numpy as np
import pytest

import device_primitive_cases as C

A_CASES = [c for c in C.CASES if c.group == "A"]
B_CASES = [c for c in C.CASES if c.group == "B"]


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def test_table_shape():
    assert [c.idx for c in C.CASES] == list(range(len(C.CASES)))
    assert {c.op for c in C.CASES} == set(C.OPS)
    assert {c.group for c in C.CASES} == set("ABCDE")
    assert {(c.grid, c.lanes) for c in A_CASES} == set(C.SHAPES) == {(c.grid, c.lanes) for c in B_CASES}
    assert 300 <= len(C.CASES) <= 2000  # a few hundred tiny launches, not tens of thousands
    assert {c.flag for c in B_CASES} == set(C.FLAGS)
    assert {c.nbytes for c in A_CASES} == set(C.COPY_BYTES + C.RAGGED_BYTES)
    for psize in (16, 8):
        for op in C.PACKET_OPS:
            assert {c.nbytes for c in B_CASES if c.op == op and c.p0 == psize} == set(C.PAYLOAD_BYTES)
    # the pattern never looks like the fill or like a flag, so a copied word is told from an untouched one
    for c in C.CASES[::7]:
        for a in range(4):
            p = C.pattern(c.idx, a, 4096)
            assert not np.isin(p, [C.FILL_WORD, 0, *C.FLAGS, *(f - 1 for f in C.FLAGS)]).any()


@pytest.mark.parametrize("op", C.COPY_OPS)
@pytest.mark.parametrize("A", C.ALIGNMENTS)
@pytest.mark.parametrize("R", (1, 0))
def test_every_copy_variant_meets_every_kind_of_case(op, A, R):
    mine = [c for c in A_CASES if (c.op, c.p0, c.p1) == (op, A, R)]
    geo = [C.copy_geometry(c) for c in mine]
    if A == 4:
        # the body's element is the 4-byte word itself: no address has a head and no size a tail
        assert all(h == 0 and t == 0 for h, b, t, _ in geo)
    else:
        assert any(h > 0 for h, *_ in geo)
        assert any(t > 0 for _, _, t, _ in geo)
        assert any("below_head" in c.tags for c in mine)
        assert any(h > 0 and t > 0 and b > 0 for h, b, t, _ in geo)  # all three loops in one call
    assert {(c.toff % 16) for c in mine} == set(C.MISALIGNMENTS)
    assert any("ragged" in c.tags and c.nbytes % 4 for c in mine)
    lanes = [(c.grid * c.lanes, c.nbytes // c.p0) for c in mine]
    assert any(n > e > 0 for n, e in lanes)  # more lanes than elements
    assert any(e > n and e % n for n, e in lanes)  # a last pass that only some lanes take
    assert any(c.grid > 1 and c.nbytes // 4 > c.lanes for c in mine)  # the flat id over several workgroups
    assert any(c.nbytes == 0 for c in mine)
    two = op in ("copy", "put2", "get2")
    assert all((c.toff != c.ooff) == two and c.toff % 16 == c.ooff % 16 and c.toff % 4 == 0 for c in mine)


def test_below_head_cases_never_reach_the_reference():
    below = [c for c in A_CASES if "below_head" in c.tags]
    assert {(c.p0, c.toff % 16, c.nbytes) for c in below} == {(16, 4, 4), (16, 4, 8), (16, 12, 0), (8, 12, 0)}
    for c in below:
        assert not c.ref
        with pytest.raises(OverflowError):
            C.expected(c, clamp=False)  # the reference's arithmetic: numInt - nFirstInt underflows
        # what the clamp means: nothing past `bytes` is written, whatever the head would have been
        L, R, K = C.expected(c)
        dst = (L, R, K)[C.copy_roles(c.op)[0]]
        assert (dst[C.GUARD + c.toff + c.nbytes:] == C.FILL).all()
    ref_lines = C.case_file_lines(for_reference=True)
    ref_idx = {int(x.split()[0]) for x in ref_lines}
    assert ref_idx == {c.idx for c in C.CASES if c.ref}
    assert not ref_idx & {c.idx for c in below}
    assert not ref_idx & {c.idx for c in C.CASES if c.op in C.LIBRARY_ONLY_OPS}
    for c in A_CASES:
        if c.ref:
            assert same(C.expected(c, clamp=False), C.expected(c))


def test_swapped_offsets_differ_on_every_two_offset_case():
    two = [c for c in C.CASES if "two_offsets" in c.tags]
    assert {c.op for c in two} == {"copy", "put2", "get2", "putPackets2", "unpackPackets2"}
    for c in two:
        assert c.toff != c.ooff and c.toff and c.ooff
        if c.nbytes // (4 if c.group == "A" or c.p0 == 8 else 8) == 0:
            continue  # nothing moves
        if c.group == "A" and not c.p1 and C.copy_geometry(c)[1] == 0:
            continue  # CopyRemainder = false and no whole element: nothing moves
        assert not same(C.expected(c, swap_offsets=True), C.expected(c)), C.format_case(c)
    assert sum(1 for c in two if not same(C.expected(c, swap_offsets=True), C.expected(c))) > len(two) * 3 // 4


def test_flipped_remainder_differs_on_every_remainder_case():
    tagged = [c for c in A_CASES if "remainder" in c.tags]
    assert len(tagged) > len(A_CASES) // 4
    for c in tagged:
        assert not same(C.expected(c, flip_remainder=True), C.expected(c)), C.format_case(c)
    for c in A_CASES:
        if "remainder" not in c.tags:
            assert same(C.expected(c, flip_remainder=True), C.expected(c))


def test_ll16_rounding_up_differs_where_four_bytes_have_no_packet():
    tagged = [c for c in B_CASES if "ll16_remainder" in c.tags]
    assert {c.nbytes for c in tagged} == {4, 12, 1028} and {c.op for c in tagged} == set(C.PACKET_OPS)
    for c in tagged:
        assert not same(C.expected(c, ll16_round_up=True), C.expected(c)), C.format_case(c)


def test_stale_units_and_packets():
    stale = [c for c in C.CASES if "stale_unit" in c.tags]
    assert {(c.p0, c.stale[0] - 8) for c in stale} == {(p, w) for p in (16, 8) for w in (1, 3, 5, 7)}
    for c in stale:
        L, R, K = C.expected(c)
        assert R[C.GUARD:C.GUARD + 8].view(np.uint32).tolist() == [1, 0]
    for c in C.CASES:
        if c.op in ("readOnce2", "readOnce3"):
            rec = C.expected(c)[0][C.GUARD + c.ooff:].view(np.uint32)
            n = 3 if c.p0 == 16 else 2
            rets = rec[0:4 * n:n].tolist()
            if c.op == "readOnce3":
                assert rets == [1, 0, 0, 0]  # ready: only the packet with both flags right
            elif c.p0 == 16:
                assert rets == [0, 1, 1, 1]  # the reference's sense: true while NOT ready
            else:
                assert rets == [0, 1, 0, 1]
    # no reader of the table is ever given a packet that is not ready to spin on
    for c in C.CASES:
        if c.stale:
            assert c.op in ("readOnce2", "readOnce3", "try_unit")


def test_guards_and_poison():
    for c in C.CASES:
        before, after = C.initial_arenas(c), C.expected(c)
        for a, (b, e) in enumerate(zip(before, after)):
            size = (c.sL, c.sR, c.sK)[a]
            assert b.size == e.size == size and 2 * C.GUARD <= size <= C.MAX_ARENA and size % 256 == 0
            d = np.flatnonzero(b != e)
            if d.size:
                assert C.GUARD <= d[0] and d[-1] < size - C.GUARD, C.format_case(c)
        for a, lo, hi in C.touched_extents(c):
            assert C.GUARD <= lo <= hi <= (c.sL, c.sR, c.sK)[a] - C.GUARD, C.format_case(c)
        if c.iK == C.INIT_IMAGE:
            end = C.GUARD + c.imgoff + c.imgcount * c.p0
            assert c.imgoff % 16 == 0 and end + C.GUARD <= c.sK
            k = before[2].view(np.uint32)
            flags = k[1::2]
            first = (C.GUARD + c.imgoff) // 4
            stale = {(first + s) // 2 for s in c.stale}
            assert all(flags[i] == c.flag for i in range(len(flags)) if i not in stale)  # every slot is valid
            outside = np.ones(len(k) // 2, bool)
            outside[first // 2:end // 8] = False
            assert (k[0::2][outside] == C.FILL_WORD).all()  # ... and outside the image it is poison


def test_case_file_round_trips(tmp_path):
    path = tmp_path / "cases.txt"
    assert C.write_case_file(str(path)) == len(C.CASES)
    lines = path.read_text().splitlines()
    assert len(lines) == len(C.CASES)
    for line, c in zip(lines, C.CASES):
        d = C.parse_case(line)
        assert d == {k: getattr(c, k) for k in d}
        assert C.format_case(C.Case(**d, group=c.group, tags=c.tags)) == line
    assert C.write_case_file(str(path), for_reference=True) == sum(c.ref for c in C.CASES)


def copy_helper_by_elements(dst, src, d_off, s_off, dst_addr, nbytes, A, R, nthreads):
    """copyHelper<T, CopyRemainder> restated lane by lane, element by element (with the clamp)."""
    num_int = nbytes // 4
    aligned = (dst_addr + A - 1) // A * A
    head = min((aligned - dst_addr) // 4, num_int)
    per = A // 4
    n_elem = (num_int - head) // per

    def copy_elems(first_byte, size, count):
        for tid in range(nthreads):
            i = tid
            while i < count:
                o = first_byte + i * size
                dst[d_off + o:d_off + o + size] = src[s_off + o:s_off + o + size]
                i += nthreads

    if R:
        copy_elems(0, 4, head)
    copy_elems(4 * head, A, n_elem)
    if R and per > 1:
        done = head + n_elem * per
        copy_elems(4 * done, 4, num_int - done)


@pytest.mark.parametrize("base", (0, 0x7F0000001000))
def test_elementwise_copy_helper_agrees_with_the_model(base):
    for c in A_CASES:
        if c.nbytes > 5000 and (c.grid * c.lanes) < 64:
            nthreads = 64  # the lane count does not change the result; keep the big single-lane cases quick
        else:
            nthreads = c.grid * c.lanes
        ar = C.initial_arenas(c)
        dst, src = C.copy_roles(c.op)
        copy_helper_by_elements(ar[dst], ar[src], C.GUARD + c.toff, C.GUARD + c.ooff, base + C.GUARD + c.toff, c.nbytes,
                                c.p0, c.p1, nthreads)
        want = C.expected(c, bases=(base,) * 3)
        assert C.first_difference(c, ar, want) is None


def test_first_difference_names_the_region():
    c = next(c for c in A_CASES if (c.op, c.p0, c.p1) == ("put2", 16, 1) and c.nbytes == 1028 and c.toff % 16 == 4)
    want = C.expected(c)
    head, body, tail, _ = C.copy_geometry(c)
    assert (head, tail) == (3, 2)
    for rel, name in ((0, "head"), (12, "body"), (12 + 16 * body, "tail"), (1028, "guard"), (-1, "guard")):
        got = [a.copy() for a in want]
        got[C.ARENA_R][C.GUARD + c.toff + rel] ^= 0xFF
        msg = C.first_difference(c, got, want)
        assert f"in {name}" in msg and C.format_case(c) in msg, msg
    assert C.first_difference(c, want, want) is None


def test_output_parser(tmp_path):
    cases = C.CASES[:3]
    blob = np.array([C.MAGIC, len(cases), 0x1000, 0x2000, 0x3000, C.GUARD, 0, 0], np.uint64).tobytes()
    for c in cases:
        blob += np.array([c.idx, c.sL, c.sR, c.sK, 0, 0, 0, 0], np.uint32).tobytes()
        blob += b"".join(a.tobytes() for a in C.expected(c))
    bases, out = C.parse_output(blob)
    assert bases == (0x1000, 0x2000, 0x3000) and sorted(out) == [0, 1, 2]
    for c in cases:
        err, arenas = out[c.idx]
        assert err == [0, 0, 0, 0] and C.first_difference(c, arenas, C.expected(c)) is None
