"""The designed part lists of tests/parts_cases.py really hold every edge they are built for, for every
codebook and start bit (CPU; tests/test_gpu_parts_edges.py walks the same lists on the device). An edge a
codebook cannot form is a failure here, never a skip."""
import numpy as np
import pytest

import parts_cases as pc

CASES = [(b, s) for b in pc.BOOKS for s in pc.START_BITS]


@pytest.mark.parametrize("name,start_bit", CASES, ids=lambda v: str(v))
def test_tiling_list_holds_every_edge(name, start_bit):
    bk, m = pc.stream(name, start_bit)
    assert m.nsym == pc.NSYM and int(bk.ln.max()) >= 3
    assert int(bk.ln[m.sym[pc.BLK - 1]]) == int(bk.ln.max())
    cuts = pc.tiling_cuts(bk, m)
    parts = pc.tiling_parts(bk, m)
    P = m.end_bit - m.start_bit
    assert cuts[0] == 0 and cuts[-1] == P and all(a < b for a, b in zip(cuts, cuts[1:]))
    assert sum(p.count for p in parts) == m.nsym
    starts = set(int(v) - m.start_bit for v in m.pos)
    width = lambda p: p.pe - p.pb  # noqa: E731
    # the parts follow each other on the true path and restore the stream
    first, entry = 0, m.start_bit
    for p in parts:
        assert (p.first, p.entry) == (first, entry)
        first, entry = first + p.count, p.exit
    assert (first, entry) == (m.nsym, m.end_bit)
    assert np.array_equal(np.concatenate([p.sym for p in parts]), m.sym)
    # no codeword start in the part: exit = entry, both at or past its end
    empty = [p for p in parts if p.count == 0]
    assert empty and all(p.entry == p.exit >= m.start_bit + p.pe for p in empty)
    assert any(p.first % pc.BLK == 0 and p.first > 0 for p in empty)            # the next codeword: a table entry
    assert any(width(p) == 1 and p.count == 1 for p in parts)
    assert any(width(p) == 1 and p.count == 0 for p in parts)
    assert any(width(p) == 1 and p.count == 0 and p.pe in starts for p in parts)   # a codeword's last bit
    assert any(p.pe in starts for p in parts) and any(p.pb in starts and p.pb > 0 for p in parts)
    # narrower than a codeword, with a start in it
    assert any(p.count == 1 and width(p) < int(bk.ln[p.sym[0]]) for p in parts)
    # 40 consecutive 1-bit parts from a codeword start, the widths in a row, part_range's 128-bit parts
    w = [width(p) for p in parts]
    run = [i for i in range(len(w) - pc.ONE_BIT_RUN + 1) if w[i:i + pc.ONE_BIT_RUN] == [1] * pc.ONE_BIT_RUN]
    assert any(parts[i].pb in starts for i in run)
    assert any(w[i:i + len(pc.WIDTHS)] == pc.WIDTHS for i in range(len(w)))
    al = [i for i in range(len(w) - pc.ALIGNED_PARTS + 1) if w[i:i + pc.ALIGNED_PARTS] == [128] * pc.ALIGNED_PARTS]
    assert any(parts[i].pb % 128 == 0 for i in al)
    assert any(width(p) > pc.LEAD_BITS for p in parts)                   # and ordinary parts
    if name == "even":
        # every codeword starts an even number of bits after the start bit, so a lead-in from an odd bit
        # never meets one: such a part's true entry comes from outside, and where the part holds no codeword
        # start that entry lies at or past its only chain's end -- at the scan and at the refix
        odd = [k for k, p in enumerate(parts) if p.count == 0 and p.pb % 2 == 1 and p.pb >= pc.LEAD_BITS]
        assert any(pc.entry_given(k) for k in odd) and any(not pc.entry_given(k) for k in odd)


@pytest.mark.parametrize("name,start_bit", CASES, ids=lambda v: str(v))
def test_slices_take_every_residue(name, start_bit):
    """Every residue of both lists occurs for every book, every pair of them too; a slice holds what the
    header asks for and never less than 16 bytes."""
    bk, m = pc.stream(name, start_bit)
    max_len = int(bk.ln.max())
    parts = pc.tiling_parts(bk, m)
    seen = set()
    for k, p in enumerate(parts):
        b0, b1, r64 = pc.slice_of(m, max_len, p.pb, p.pe, k)
        assert 0 <= b0 and b1 <= m.payload.size and b1 - b0 >= 16
        assert 8 * b0 <= m.start_bit + p.pb - min(pc.LEAD_BITS, p.pb)
        assert 8 * b1 >= min(m.start_bit + p.pe + max_len, 8 * m.payload.size)
        assert b0 >= (m.start_bit + p.pb - min(pc.LEAD_BITS, p.pb)) // 8 - 15      # the least range, lowered by < 16
        seen.add((b0 % 16, r64))
    assert {a for a, _ in seen} >= set(pc.R16) and {b for _, b in seen} == set(pc.R64)
    assert seen >= {(a, b) for a in pc.R16 for b in pc.R64}
    # the offset between a stream bit and its bit in the 64-byte aligned view, modulo 128 bits: not only 0
    assert len({(8 * r64 - 8 * r16) % 128 for r16, r64 in seen}) >= 12


@pytest.mark.parametrize("name", pc.BOOKS)
def test_last_width_and_padding_parts(name):
    start_bit = pc.START_BITS[pc.BOOKS.index(name) % 2]
    bk, m = pc.stream(name, start_bit, pc.WAVES)
    parts = pc.last_width_parts(m)
    P = m.end_bit - m.start_bit
    assert len(parts) == pc.LAST_WIDTHS == 128 and parts[-1].pe == P - 1
    assert {p.pe % 128 for p in parts} == set(range(128)) and all(p.pb == 0 and p.first == 0 for p in parts)
    assert all(p.entry == m.start_bit for p in parts)
    assert all(a.count <= b.count for a, b in zip(parts, parts[1:])) and parts[-1].count >= m.nsym - 1
    for s in pc.START_BITS:
        bk, m = pc.stream(name, s)
        pad = pc.padding_part(bk, m, pc.tiling_cuts(bk, m)[-2])
        assert pad.pe == 8 * m.payload.size - s and pad.exit >= s + pad.pe and pad.count >= m.nsym - pad.first > 0
