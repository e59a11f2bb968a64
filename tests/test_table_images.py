"""Every device table image that hz_codebook.cpp builds, checked entry by entry on the CPU.

tests/table_probe.cpp (built here once per session with plain hipcc; it links hz_codebook.cpp only and
makes no HIP call) builds the images of a codebook exactly as the uploads decide to. For every book of
tests/table_books.py and for EVERY symbol of the book, the codeword followed by eight suffix patterns
(all zeros, all ones, four seeded random suffixes, the book's shortest code, its longest code) goes
through every resolver of tests/table_model.py -- the numpy restatement of what each kernel does with
an image -- and must come back as the symbol and its length: the LUT in its 64-bit and 32-bit forms,
DENSE and FIXED16 decode, the HOT slots with their escapes and an independent choice of the pairing
mask, the DENSE / WIDE / FIXED16 encode images, len8, lenpair, the index walker and the chain walker with
its DEEP escapes. Then the invariants the kernels rely on without checking: link targets inside their
tables, no LDS link in a head, leaves that read as out-of-range links and LDS addresses, fillers, sizes
and padding, the LDS budget, and the pipelined decoders' hop bound (table_model.PIPE_GLOBAL_HOPS).

Books: 7 designed + zipf21 + sq32 + ragged + 3 small + 2 foreign + 64 seeded random = 79; the whole file
takes about half a minute on one CPU core (and a few seconds to build the probe). The probe's sanitized build (its header comment) is a manual CPU
step, not a test. Tolerance: none -- everything is exact."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import table_books  # noqa: E402
import table_model as tm  # noqa: E402

LEAF_1_0 = (1 << 31) | (1 << 24)


# ---- the probe ----------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def probe(built_lib, tmp_path_factory):
    from huffman_amd import build
    exe = str(tmp_path_factory.mktemp("table_probe") / "table_probe")
    src = [os.path.join(ROOT, "tests", "table_probe.cpp"), os.path.join(ROOT, "huffman_amd", "csrc", "hz_codebook.cpp")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "huffman_amd", "csrc")]
    r = subprocess.run([build.HIPCC, "-O1", "-std=c++17"] + inc + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def write_book(path, bk):
    used = bk.ln[bk.ln > 0]
    with open(path, "wb") as f:
        f.write(struct.pack("<III", used.size, int(used.min()), int(used.max())))
        f.write(bk.ln.astype(np.uint8).tobytes())
        f.write(bk.code.astype("<u8").tobytes())


def read_images(path):
    """{section: (params, words)} of a probe output."""
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:8] == b"HZTP0001"
    at, out = 8, {}
    while at < len(blob):
        name = blob[at:at + 24].rstrip(b"\0").decode()
        nparam, wb, nwords = struct.unpack_from("<IIQ", blob, at + 24)
        at += 40
        params = {}
        for _ in range(nparam):
            params[blob[at:at + 24].rstrip(b"\0").decode()] = struct.unpack_from("<q", blob, at + 24)[0]
            at += 32
        words = np.frombuffer(blob, dtype="<u%d" % wb, count=nwords, offset=at).copy()
        at += wb * nwords
        assert name not in out
        out[name] = (params, words)
    assert at == len(blob)
    return out


_images = {}


def images(probe, tmp_path_factory, name):
    if name not in _images:
        d = tmp_path_factory.mktemp("book_" + name)
        bk = table_books.book(name)
        write_book(str(d / "book.bin"), bk)
        r = subprocess.run([probe, str(d / "book.bin"), str(d / "images.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _images[name] = read_images(str(d / "images.bin"))
    return _images[name]


# ---- the checks ---------------------------------------------------------------------------------
def suffixes(bk, syms, seed):
    """(name, u64 suffix per symbol): zeros, ones, four seeded random, the shortest and the longest code."""
    rng = np.random.default_rng(seed)
    used = np.nonzero(bk.ln)[0]
    shortest = used[np.argmin(bk.ln[used])]
    longest = used[np.argmax(bk.ln[used])]
    out = [("zeros", np.uint64(0)), ("ones", np.uint64((1 << 64) - 1))]
    out += [("random%d" % i, rng.integers(0, 1 << 64, syms.size, dtype=np.uint64)) for i in range(4)]
    out.append(("shortest", tm.prefix_bits(bk.ln, bk.code, shortest)))                                  # then zeros
    out.append(("longest", tm.prefix_bits(bk.ln, bk.code, longest) | np.uint64((1 << (64 - int(bk.ln[longest]))) - 1)))
    return out


def expect(what, syms, got_sym, got_len, want_len, unit=" bits"):
    """Every window resolves to its symbol and length; names the first symbol that does not."""
    bad = (got_len != want_len) if got_sym is None else ((got_sym != syms) | (got_len != want_len))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: symbol 0x%04x (%d%s) resolved as %s, %d%s" % (
            what, int(syms[i]), int(want_len[i]), unit, "-" if got_sym is None else "0x%04x" % int(got_sym[i]),
            int(got_len[i]), unit))


def check_lut_structure(what, bk, img, l2, k1, lvl):
    """What the decoders assume of a LUT's images without checking."""
    max_len = int(bk.ln.max())
    n1 = 1 << k1
    assert k1 == max(1, min(max_len, tm.K_DEC_LUT_MAX_K1)), what
    assert 4 <= lvl <= tm.K_DEC_LEVEL_BITS, what
    assert img.size % 4 == 0 and img.size >= max(n1, tm.K_DEC_MIN_LDS_WORDS), what       # copy_lds_table: uint4s
    assert 1 <= l2.size <= tm.K_LUT_MAX_L2, what
    for tab, tname in ((img, "lds"), (l2, "l2")):
        leaf = (tab >> np.uint32(31)) == 1
        raw = (tab >> np.uint32(10)).astype(np.int64)
        nb = ((tab >> np.uint32(5)) & np.uint32(15)).astype(np.int64)
        width = ((tab >> np.uint32(5)) & np.uint32(31)).astype(np.int64)
        where = "%s %s[%%d] = 0x%%08x: " % (what, tname)

        def none(bad, text):
            if bad.any():
                i = int(np.nonzero(bad)[0][0])
                L, s = (int(tab[i]) >> 24) & 63, (int(tab[i]) >> 8) & 0xffff
                raise AssertionError((where % (i, int(tab[i]))) + text + " (as a leaf: symbol 0x%04x, %d bits)" % (s, L))
        link = ~leaf
        lds_link = link & (raw < tm.K_LUT_GLOBAL)
        none(link & (nb == 0), "a link of no index bits (or an unfilled entry)")
        none(link & (width != nb), "a link wider than 15 bits")
        if tname == "lds":
            head = np.arange(tab.size) >= n1
            none(lds_link & head, "a head entry that is itself an LDS link: the pipelined form takes one LDS hop")
            none(lds_link & ((raw < n1) | (raw + (1 << nb) > tab.size)), "an LDS link's target range leaves the LDS image")
        else:
            none(lds_link, "an LDS link in the global table")
        g = link & ~lds_link
        none(g & (raw - tm.K_LUT_GLOBAL + (1 << nb) > l2.size), "a global link's target range leaves l2")
        none(g & (nb > lvl), "a global subtable wider than the level bits")
        # leaves: the claims at lut_leaf_entry and lut_l2_rsrc
        L = ((tab >> np.uint32(24)) & np.uint32(63)).astype(np.int64)
        sym = ((tab >> np.uint32(8)) & np.uint32(0xffff)).astype(np.int64)
        none(leaf & ((tab & np.uint32(0xff)) != 0), "a leaf with a bit set in bits 7..0")
        none(leaf & ((tab >> np.uint32(30)) & np.uint32(1) != 0), "a leaf with bit 30 set")
        none(leaf & ~(((L == bk.ln[sym]) & (L > 0)) | ((L == 1) & (sym == 0))), "a leaf of no code of the book")
        none(leaf & ((tab & np.uint32(31)) != 0), "a leaf whose pos field is not 0")
        none(leaf & (raw < (1 << 21)), "a leaf that reads as a link below index 2^21")
        none(leaf & ((raw + (1 << width) - 1) * 4 >= (1 << 27)), "a leaf whose byte offset as a link reaches 2^27")
        none(leaf & (raw * 4 < tm.K_LDS_BYTES), "a leaf that reads as an LDS address inside the LDS")
    # unused level-1 windows (incomplete codes) hold the 1-bit filler
    unused = ~tm.touched(bk.ln, bk.code, k1)
    assert (img[:n1][unused] == LEAF_1_0).all(), what + ": an unused level-1 window without the filler"
    # the LDS budget: the table, then kDecMaxWaves staging slots of the estimated block
    slots = 4 * tm.K_DEC_MAX_WAVES * tm.dec_slot_words(tm.est_bits(bk.ln), max_len)
    assert 4 * img.size + slots <= tm.K_LDS_BYTES, what + ": the LDS image and its staging slots exceed the LDS"
    assert 4 * img.size + 4 * tm.dec_slot_words(tm.K_BLOCK_SYMS * max_len, max_len) <= tm.K_LDS_BYTES, what


def check_lut(what, bk, syms, L, wins, gaps, img, l2, k1, lvl):
    max_len = int(bk.ln.max())
    check_lut_structure(what, bk, img, l2, k1, lvl)
    pipe = tm.pipelined(max_len, k1, lvl)
    hops_max = 0
    for sname, w64 in wins:
        s64, l64, hops = tm.lut64(img, l2, k1, w64, syms)
        expect("%s 64-bit form, suffix %s" % (what, sname), syms, s64, l64, L)
        hops_max = max(hops_max, int(hops.max()))
        if max_len <= 32:     # the 32-bit forms run for these codebooks only (pos covers 32-bit windows)
            s32, l32, lh, gh = tm.lut32(img, l2, k1, tm.top32(w64), syms)
            expect("%s 32-bit form, suffix %s" % (what, sname), syms, s32, l32, L)
            assert (lh <= tm.PIPE_LDS_HOPS).all()
            if pipe:
                bad = gh > tm.PIPE_GLOBAL_HOPS
                assert not bad.any(), "%s: symbol 0x%04x takes %d global hops in a pipelined decoder" % (
                    what, int(syms[np.nonzero(bad)[0][0]]), int(gh.max()))
    if gaps.size:             # unused code space: the 1-bit filler of symbol 0, in every level
        gs, gl, _ = tm.lut64(img, l2, k1, gaps)
        assert (gs == 0).all() and (gl == 1).all(), what + ": an unused window without the filler leaf(1, 0)"
        if max_len <= 32:
            gs, gl, _, gh = tm.lut32(img, l2, k1, tm.top32(gaps))
            assert (gs == 0).all() and (gl == 1).all(), what + ": 32-bit form, unused window"
            assert not pipe or (gh <= tm.PIPE_GLOBAL_HOPS).all()
    return hops_max


def check_bytes_fill(what, bk, table8, bits, filler):
    unused = ~tm.touched(bk.ln, bk.code, bits)
    assert (table8[:1 << bits][unused] == filler).all(), "%s: an unused window without the filler %d" % (what, filler)


def check_book(bk, im):
    """Every image of one book; returns facts the named books assert."""
    ln, code = bk.ln, bk.code
    syms = np.nonzero(ln)[0].astype(np.int64)
    L = ln[syms].astype(np.int64)
    min_len, max_len = int(L.min()), int(L.max())
    facts = {}
    wins = [(n, tm.windows64(ln, code, syms, suf)) for n, suf in suffixes(bk, syms, 1000 + syms.size)]
    g = tm.gaps64(ln, code)
    gaps = np.array([v for lo, hi in g[:20000] for v in (lo, hi, lo + (hi - lo) // 2)], dtype=np.uint64)
    for k, v in im["consts"][0].items():    # the model's constants are the headers'
        assert tm.CONSTS[k] == v, k

    # ---- encode ----
    enc = im["enc"][0]["mode"]
    want_enc = (tm.ENC_FIXED16 if (min_len, max_len) == (16, 16) else tm.ENC_DENSE if max_len <= 16
                else tm.ENC_HOT if max_len <= tm.K_HOT_MAX_LEN else tm.ENC_WIDE)
    assert enc == want_enc
    facts["enc"] = enc
    for sec in ("enc_fixed16", "enc_dense", "enc_hot", "enc_esc", "enc_wide"):
        assert (sec in im) == (sec in {tm.ENC_FIXED16: ["enc_fixed16"], tm.ENC_DENSE: ["enc_dense"],
                                       tm.ENC_HOT: ["enc_hot", "enc_esc"], tm.ENC_WIDE: ["enc_wide"]}[enc]), sec
    if enc == tm.ENC_FIXED16:
        img = im["enc_fixed16"][1]
        assert img.size == 65536 * 2 // 4
        expect("FIXED16 encode", syms, None, img.view("<u2")[syms].astype(np.int64), code[syms].astype(np.int64), unit=" (code)")
    elif enc == tm.ENC_DENSE:
        img = im["enc_dense"][1]
        assert img.size == (65536 * 17 // 8 + 16) // 4 and img.size % 4 == 0
        dl, dc = tm.dense_encode(img, np.arange(65536))
        expect("DENSE encode length", np.arange(65536), None, dl, ln.astype(np.int64))
        expect("DENSE encode code", np.arange(65536), None, dc, code.astype(np.int64), unit=" (code)")
    elif enc == tm.ENC_HOT:
        (p, img), (_, esc) = im["enc_hot"], im["enc_esc"]
        mask = p["mask"]
        assert img.size == 32768 and esc.size == 32768
        miss = [tm.hot_miss_mass(ln, m) for m in tm.HOT_MASKS]
        assert mask == tm.HOT_MASKS[int(np.argmin(miss))], "pairing mask 0x%04x is not the first minimum of %s" % (mask, miss)
        hl, hc, hit = tm.hot_lookup(img, esc, mask, syms)
        expect("HOT length", syms, None, hl, L)
        expect("HOT code", syms, None, hc, code[syms].astype(np.int64), unit=" (code)")
        owns = tm.hot_owner(ln, mask)
        bad = hit != owns[syms]
        assert not bad.any(), "HOT slot of symbol 0x%04x: owner against the rule (shorter code, then below 0x8000)" % int(
            syms[np.nonzero(bad)[0][0]])
        a = np.arange(32768)
        empty = ~owns[a] & ~owns[a ^ (mask & 0x7fff) ^ 0x8000]
        assert (img[tm.hot_word(a)][empty] == 0).all(), "an empty HOT slot is not 0"
        facts["mask"], facts["misses"] = mask, int((~hit).sum())
    else:
        img = im["enc_wide"][1]
        assert img.size == 65536 and img.dtype.itemsize == 8
        wl, wc = tm.wide_encode(img, np.arange(65536))
        expect("WIDE length", np.arange(65536), None, wl, ln.astype(np.int64))
        expect("WIDE code", np.arange(65536), None, wc.astype(np.int64), code.astype(np.int64), unit=" (code)")
    assert ("len8" in im) == ("lenpair" in im) == (enc != tm.ENC_FIXED16)
    if enc != tm.ENC_FIXED16:
        assert im["len8"][1].size == 16384 and im["lenpair"][1].size == 16384
        every = np.arange(65536)
        expect("len8", every, None, tm.len8_lookup(im["len8"][1], every), ln.astype(np.int64))
        expect("lenpair", every, None, tm.lenpair_lookup(im["lenpair"][1], every), ln.astype(np.int64))

    # ---- decode ----
    dp = im["dec"][0]
    dec = dp["mode"]
    assert dp["rc"] == 0
    dense_words = lambda k: 4 * (((max((1 << k) // 2, 1) + max((1 << k) // 16, 1)) + 3) & ~3)  # noqa: E731
    want_dec = (tm.DEC_FIXED16 if (min_len, max_len) == (16, 16) else
                tm.DEC_DENSE if max_len <= 16 and max_len - min_len <= 3 and
                dense_words(max_len) + 4 * tm.K_DEC_MIN_WAVES * tm.dec_slot_words(tm.K_BLOCK_SYMS * max_len, max_len) <= tm.K_LDS_BYTES
                else tm.DEC_LUT)
    assert dec == want_dec
    facts["dec"] = dec
    lut = None
    if dec == tm.DEC_FIXED16:
        img = im["dec_fixed16"][1]
        assert img.size == 32768 and im["dec_fixed16"][0]["k"] == 16
        for sname, w64 in wins:
            expect("FIXED16 decode, suffix " + sname, syms, *tm.fixed16_decode(img, w64), L)
        for sec in ("walk_len", "walk_esc", "walk8", "chain_esc", "chain_lut"):
            assert sec not in im, sec
        return facts
    if dec == tm.DEC_DENSE:
        p, img = im["dec_dense"]
        assert p["k"] == max_len and img.size * 4 == dense_words(max_len)
        for sname, w64 in wins:
            expect("DENSE decode, suffix " + sname, syms, *tm.dense_decode(img, p["k"], min_len, w64), L)
        unused = ~tm.touched(ln, code, max_len)
        assert (img.view("<u2")[:1 << max_len][unused] == 0).all()
        cp, cimg = im["chain_lut"]
        assert cp["rc"] == 0
        lut = ("chain LUT", cimg, im["chain_l2"][1], cp["k"], cp["lvl"])
    else:
        p, img = im["dec_lut"]
        assert "chain_lut" not in im
        lut = ("LUT", img, im["dec_l2"][1], p["k"], p["lvl"])
    facts["k1"], facts["lvl"] = lut[3], lut[4]
    facts["hops"] = check_lut(lut[0], bk, syms, L, wins, gaps, *lut[1:])
    facts["lds_words"], facts["l2_entries"] = lut[1].size, lut[2].size
    links = np.concatenate([lut[1], lut[2]])
    links = links[(links >> np.uint32(31)) == 0]
    facts["nb_max"] = int(((links >> np.uint32(5)) & np.uint32(15)).max()) if links.size else 0

    # ---- the index walker ----
    walker = "walk_len" in im
    K = max(2, min(max_len, tm.K_WALK_K, min_len + 14))
    assert walker == (max_len <= tm.K_WALK_MAX_LEN and max(1 << (K - 1), 16) <= (1 << tm.K_WALK_K) // 2)
    if walker:
        (p, wimg), (_, wesc) = im["walk_len"], im["walk_esc"]
        k, m, bias = p["k"], p["m"], p["bias"]
        assert (k, m, bias) == (K, max_len, min_len - 1)
        assert wimg.size * 4 == max(1 << (k - 1), 16) and wimg.size % 4 == 0
        assert wesc.size == ((1 << m) // 4 if m > min(k, 16) else 1)
        for sname, w64 in wins:
            wl, escd = tm.idx_walk(wimg, wesc, k, m, bias, tm.top32(w64))
            expect("index walker, suffix " + sname, syms, None, wl, L)
            assert not (escd & (L <= k)).any(), "a code within the walker's window escapes"
        nibbles = np.stack([wimg.view(np.uint8) & 15, wimg.view(np.uint8) >> 4], axis=1).reshape(-1)
        check_bytes_fill("index walker table", bk, nibbles, k, 1)             # nibble 1 + bias = min_len
        if wesc.size > 1:
            check_bytes_fill("index walker escapes", bk, wesc.view(np.uint8), m, 1)
        if gaps.size:
            wl, _ = tm.idx_walk(wimg, wesc, k, m, bias, tm.top32(gaps))
            assert (wl >= 1).all(), "an unused window stalls the index walk"
        facts["walk"] = (k, m, bias)

    # ---- the chain walker ----
    (p8, w8), (pe, cesc) = im["walk8"], im["chain_esc"]
    k8, m = p8["k"], pe["m"]
    assert k8 == max(1, min(max_len, 16)) and w8.size * 4 == (((1 << k8) + 15) & ~15)
    assert (w8.view(np.uint8)[1 << k8:] == 0).all()
    assert pe["shared"] == int(walker)
    if walker:
        cesc = im["walk_esc"][1]
    else:
        assert m == min(max_len, tm.K_CHAIN_ESC_MAX_BITS) and cesc.size * 4 == (((1 << m) + 15) & ~15)
        assert (cesc.view(np.uint8)[1 << m:] == 1).all()
        unused = ~tm.touched(ln, code, m)
        assert (cesc.view(np.uint8)[:1 << m][unused] == 1).all(), "chain escapes: an unused window without the filler 1"
    check_bytes_fill("chain walker table", bk, w8.view(np.uint8), k8, min_len)
    # a DEEP 0 is legal only under an m-bit prefix shared by codes of different lengths longer than m
    longer = L > m
    pre, inv = np.unique((code[syms[longer]] >> (L[longer] - m).astype(np.uint64)).astype(np.int64), return_inverse=True)
    lo = np.full(pre.size, 255, np.int64)
    hi = np.zeros(pre.size, np.int64)
    np.minimum.at(lo, inv, L[longer])
    np.maximum.at(hi, inv, L[longer])
    ndeep = 0
    for sname, w64 in wins:
        W = tm.top32(w64)
        cl, escd, deep = tm.chain_walk(w8, k8, cesc, m, W)
        if deep.any():
            pw = (W[deep] >> np.uint32(32 - m)).astype(np.int64)
            at = np.minimum(np.searchsorted(pre, pw), max(pre.size - 1, 0))
            bad = ~((pre[at] == pw) & (hi[at] > lo[at])) if pre.size else np.ones(pw.shape, bool)
            assert not bad.any(), "chain walker: DEEP escape of symbol 0x%04x under a prefix of one length" % int(
                syms[deep][np.nonzero(bad)[0][0]])
            assert max_len > m
            cl = np.where(deep, tm.lut64(lut[1], lut[2], lut[3], w64, syms)[1], cl)   # deep_len: the LUT's 64-bit form
            ndeep = max(ndeep, int(deep.sum()))
        expect("chain walker, suffix " + sname, syms, None, cl, L)
        assert not (escd & (L <= k8)).any(), "a code within the byte table's window escapes"
    if gaps.size:
        cl, _, deep = tm.chain_walk(w8, k8, cesc, m, tm.top32(gaps))
        assert ((cl >= 1) | deep).all() and (not deep.any() or max_len > m), "an unused window stalls the chain walk"
    facts["k8"], facts["chain_esc_m"], facts["deep"] = k8, m, ndeep
    return facts


# ---- the tests ----------------------------------------------------------------------------------
_facts = {}


def facts(probe, tmp_path_factory, name):
    if name not in _facts:
        _facts[name] = check_book(table_books.book(name), images(probe, tmp_path_factory, name))
    return _facts[name]


@pytest.mark.parametrize("name", table_books.ALL)
def test_table_images(probe, tmp_path_factory, name):
    facts(probe, tmp_path_factory, name)


def test_zipf21_is_the_benchmark_class(probe, tmp_path_factory):
    f = facts(probe, tmp_path_factory, "zipf21")
    assert (f["enc"], f["dec"]) == (tm.ENC_HOT, tm.DEC_LUT)
    assert f["mask"] == 0xffff and f["misses"] >= 65536 // 4
    assert (f["k1"], f["lvl"]) == (13, 12)
    assert 20000 < f["lds_words"] <= tm.K_LDS_BYTES // 4 and 250000 < f["l2_entries"] < 300000   # heads; the global levels
    assert f["walk"] == (17, 21, 4) and f["hops"] == 2     # an LDS head, then one global subtable


def test_sq32_is_wide_with_deep_escapes(probe, tmp_path_factory):
    f = facts(probe, tmp_path_factory, "sq32")
    assert (f["enc"], f["dec"]) == (tm.ENC_WIDE, tm.DEC_LUT)
    assert f["hops"] == 3 and "walk" not in f
    assert f["chain_esc_m"] == 25 and f["deep"] > 0


def test_caterpillars_narrow_the_global_levels(probe, tmp_path_factory):
    f = facts(probe, tmp_path_factory, "cat4096")
    assert f["dec"] == tm.DEC_LUT and f["lvl"] < 12
    assert not tm.pipelined(22, f["k1"], f["lvl"])          # 22-bit codes past 13 + lvl bits: the looping decoders


def test_ragged_ties_make_narrow_subtables(probe, tmp_path_factory):
    f = facts(probe, tmp_path_factory, "ragged")
    assert f["dec"] == tm.DEC_LUT and f["k1"] == 13 and 1 <= f["nb_max"] <= 4
