"""GPU suite: the key half of aggregate verification in GT, value by value.

The tables (bn256_gttab.hip: k_gt_keys, k_gt_nib, k_gt_cross, k_gt_win16,
k_gt_blocks, k_tor_scan, k_tor_convert) and the fold (bn256_gt.hip: k_gt_plan,
k_gt_chunks, k_tor_chunks, k_gt_combine) are read back raw (hg_debug_gt_layout,
hg_debug_gt_entries, hg_debug_gt_fold) and compared word for word with the
integer model of tests/_gt_model.py, which tests/test_gt_model.py proves on the
CPU: registry keys are k_i G2Base, every table value is g^(sum of k_i) with
g = FE(Miller(G2Base, H)), the fold's Y is conj(g^K).

Tables: 17 keys (a one-key second 16-key window without an upper 8-key window;
level 4 has a clipped block), 25 keys (a ragged upper 8-key window), 33 keys
with ks[3] = r - ks[2] (a degenerate entry: the set stays in Fp12 form). All
keys, all 8-key entries and all blocks are compared; of each 16-key window every
entry whose low or high byte is 0x00, 0x01, 0x80 or 0xFF plus 4096 seeded ones
(about 5900 per window; in a ragged window the entries the conversion skips are
among them and must be the Fp12 bytes of 1). The expected words of all 65536
entries of the 17-key registry's full window measured 4 s of Python in Fp12
form and 16 s in torus form (one CPU core), against 0.5 s and 1.8 s for the
sample: not "a few seconds", so the sample stands. The Fp12 form of the 17- and 25-key
registries: keys, 8-key windows and blocks from a level-1 build of the same
registry (then level 2 is built on top, and keys and 8-key windows must come
back unchanged); the 16-key windows from their degenerate twin (the same
registry with ks[3] = r - ks[2], which the scan leaves unconverted), in
process: no HG_GT_TORUS=0 child.

Fold: 224 keys (14 sixteen-key windows, the smallest registry with 13 or more
terms), one corpus of 41 requests (tests/_gt_model.py fold_corpus), folded with
1, 2, 3, 8, 13 and 16 terms per chunk over the converted set, over its
degenerate twin (Fp12 form, 16-key windows) and at level 1 (8-key windows, up
to 28 terms), plus a call with one request.
"""

import functools

import numpy as np
import pytest

from handel_amd.engine import REQ_DTYPE, Engine
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _gt_model as M

pytestmark = pytest.mark.gpu

MSG = F.LIB_MESSAGE
ONE = M.fe_words(O.F12_ONE)


@pytest.fixture(scope="module", params=["go", "cf"])
def eng(request):
    e = Engine(device=0, flavor=request.param)
    e.flavor_name = request.param
    e.set_aggregate_level(2)
    yield e
    e.close()


def _load(e, ks, level=2):
    """The registry k_i G2Base with its tables built up to `level`."""
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not e.registry_load(reg).any()
    e.set_aggregate_level(level)
    try:
        assert e.prepare_aggregate_msg(MSG) == 0 and e.aggregate_tables() == level
    finally:
        e.set_aggregate_level(2)
    return reg


# ------------------------------------------------------------------ expected tables (computed once, shared by the flavors)
@functools.lru_cache(maxsize=None)
def _model(nreg, degenerate):
    base = F.scalars(nreg, seed=b"gt-values-%d" % nreg)
    return M.TableModel(M.table_scalars(base, degenerate), M.generator_value(MSG))


@functools.lru_cache(maxsize=None)
def _want_small(nreg, degenerate):
    """Keys, every 8-key entry and every block, in Fp12 form: {table: words (n, 120)}, blocks in table order."""
    m = _model(nreg, degenerate)
    blocks = [(k, j) for k in range(4, m.levels + 1) for j in range(m.block_count(k))]
    return {"keys": np.stack([M.fe_words(v) for v in m.keys]),
            "win8": np.stack([M.fe_words(v) for w in range(m.nwin8) for v in m.win8(w)]),
            "blocks": np.stack([M.fe_words(m.block(k, j)) for k, j in blocks]), "block_ids": blocks}


@functools.lru_cache(maxsize=None)
def _want_blocks_torus(nreg):
    m = _model(nreg, False)
    return np.stack([M.torus_words(m.block(k, j)) for k, j in _want_small(nreg, False)["block_ids"]])


@functools.lru_cache(maxsize=None)
def _want_win16(nreg, degenerate, w, torus):
    """(subsets, words) of the sampled entries of 16-key window w; a skipped entry of a converted set is 1."""
    m = _model(nreg, degenerate)
    have = min(16, nreg - 16 * w)
    S = M.window_samples(nreg, w)
    memo = {}
    rows = []
    for s in S:
        key = s & ((1 << have) - 1)  # absent keys count as 1: the value depends on the window's keys alone
        if key not in memo:
            v = m.win16(w, s)
            assert v == m.win16(w, key)
            memo[key] = M.torus_words(v) if torus and key else M.fe_words(v)
        rows.append(memo[key])
        if torus and M.skipped(nreg, w, s):
            assert (rows[-1] == ONE).all()
    return S, np.stack(rows)


def _compare(table, got, want, name):
    """Word for word; a failure names table, entry (name(i)) and element."""
    assert got.shape == want.shape, (table, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        i, word = (int(x) for x in bad[0])
        rows = sorted({int(r) for r, _ in bad})
        pytest.fail(f"{table}: {name(i)}, element {word // 10} (word {word}): got {got[i, word]:#x}, want "
                    f"{want[i, word]:#x}; {len(rows)} of {len(got)} entries differ, first {[name(r) for r in rows[:6]]}")


def _check_layout(e, m, level, torus):
    lay = e.gt_layout()
    assert (lay["level"], lay["torus"], lay["nreg"], lay["nwin8"], lay["nwin16"]) == (level, torus, m.nreg, m.nwin8,
                                                                                       m.nwin16)
    base, want = 0, {}
    for k in range(4, m.levels + 1):
        want[k] = (base, m.block_count(k))
        base += m.block_count(k)
    assert lay["blocks"] == want
    return base


def _check_small(e, nreg, degenerate, blocks_torus):
    """All keys, all 8-key entries, all blocks of the loaded set."""
    m, want = _model(nreg, degenerate), _want_small(nreg, degenerate)
    keys = e.gt_entries(e.GT_KEYS, 0, nreg)
    w8 = e.gt_entries(e.GT_WIN8, 0, 256 * m.nwin8)
    blk = e.gt_entries(e.GT_BLOCKS, 0, len(want["block_ids"]))
    _compare("keys", keys, want["keys"], lambda i: f"key {i}")
    _compare("8-key windows", w8, want["win8"], lambda i: f"window {i // 256}, subset {i % 256:#04x}")
    _compare("blocks (torus)" if blocks_torus else "blocks", blk,
             _want_blocks_torus(nreg) if blocks_torus else want["blocks"],
             lambda i: "block (level %d, %d)" % want["block_ids"][i])
    return keys, w8


def _check_win16(e, nreg, degenerate, torus):
    m = _model(nreg, degenerate)
    for w in range(m.nwin16):
        S, want = _want_win16(nreg, degenerate, w, torus)
        got = e.gt_entries(e.GT_WIN16, 65536 * w, 65536)[S]
        form = "torus" if torus else "Fp12"
        _compare(f"16-key windows ({form}, {nreg} keys)", got, want,
                 lambda i: f"window {w}, subset {S[i]:#06x}" + (" (skipped)" if M.skipped(nreg, w, S[i]) else ""))


@pytest.mark.parametrize("nreg", [17, 25])
def test_tables_fp12_then_torus(eng, nreg):
    """Level 1 of the registry (Fp12 blocks), level 2 on top of it (converted:
    keys and 8-key windows unchanged, 16-key windows and blocks in torus form,
    the ragged window's skipped entries still 1)."""
    m = _model(nreg, False)
    _load(eng, m.ks, level=1)
    nblk = _check_layout(eng, m, 1, False)
    assert nblk == len(_want_small(nreg, False)["block_ids"])
    keys1, w8_1 = _check_small(eng, nreg, False, blocks_torus=False)
    assert eng.prepare_aggregate() == 0 and eng.aggregate_tables() == 2 and eng.aggregate_tables_torus()
    _check_layout(eng, m, 2, True)
    keys2, w8_2 = _check_small(eng, nreg, False, blocks_torus=True)
    assert (keys1 == keys2).all() and (w8_1 == w8_2).all()
    _check_win16(eng, nreg, False, torus=True)


@pytest.mark.parametrize("nreg", [17, 25, 33])
def test_tables_of_a_degenerate_registry_stay_fp12(eng, nreg):
    """ks[3] = r - ks[2]: the scan finds subset 0x000c of window 0 (and what
    contains only it), nothing is converted, and every table is the Fp12 value:
    the 33-key registry of the issue, and the Fp12 twins of the other two."""
    m = _model(nreg, True)
    assert (m.ks[2] + m.ks[3]) % O.ORDER == 0 and O.f12_is_one(m.win16(0, 0x000C))
    _load(eng, m.ks)
    assert not eng.aggregate_tables_torus()
    _check_layout(eng, m, 2, False)
    _check_small(eng, nreg, True, blocks_torus=False)
    _check_win16(eng, nreg, True, torus=False)


# ------------------------------------------------------------------ the fold
@functools.lru_cache(maxsize=None)
def _fold_case(degenerate):
    """ks, reqs, words, labels, codes and per request the expected Y (None for the two error cases)."""
    ks = M.fold_scalars(F.scalars(M.FOLD_NREG, seed=b"gt-values-224"), degenerate)
    reqs, words, labels = M.fold_corpus()
    g = M.generator_value(MSG)
    codes = [M.fold_code(r, words, M.FOLD_NREG) for r in reqs]
    ys = [M.fold_value(g, M.fold_scalar(ks, r, words)) if c == M.HG_OK else None for r, c in zip(reqs, codes)]
    return ks, np.array(reqs, dtype=REQ_DTYPE), words, labels, np.array(codes, dtype=np.int32), ys


def _loaded(e, tag, ks, level=2):
    """The 224-key tables are built once per form and flavor."""
    if getattr(e, "_gt_values_tag", None) != (tag, e.flavor_name):
        e._gt_values_tag = None
        _load(e, ks, level)
        e._gt_values_tag = (tag, e.flavor_name)


def _fold_all(e, reqs, words):
    return {chunk: e.gt_fold(reqs, words, chunk) for chunk in M.CHUNKS}


def _check_fp12_fold(e, degenerate, what):
    _, reqs, words, labels, codes, ys = _fold_case(degenerate)
    ok = [i for i, c in enumerate(codes) if c == M.HG_OK]
    assert len(ok) == len(reqs) - 2
    want = np.stack([M.fe_words(ys[i]) for i in ok])
    for chunk, (y, got_codes) in _fold_all(e, reqs, words).items():
        assert list(got_codes) == list(codes), chunk
        assert not y[codes != M.HG_OK].any()
        _compare(f"{what}, chunk {chunk}", y[ok], want, lambda i: f"request {ok[i]} ({labels[ok[i]]})")
    i = labels.index("fourteen-terms")  # n = 1
    y, got_codes = e.gt_fold(reqs[i:i + 1], words, 8)
    assert list(got_codes) == [0] and (y[0] == M.fe_words(ys[i])).all()


def test_fold_values_torus(eng):
    """Over the converted set the fold leaves X with X/conj(X) = Y: canonical,
    nonzero, X == Y conj(X) in integers, and, the product being commutative
    and every program output canonical, the same words for every chunk size."""
    ks, reqs, words, labels, codes, ys = _fold_case(False)
    _loaded(eng, "torus", ks)
    assert eng.aggregate_tables_torus()
    runs = _fold_all(eng, reqs, words)
    ok = [i for i, c in enumerate(codes) if c == M.HG_OK]
    assert sorted(set(range(len(reqs))) - set(ok)) == sorted([labels.index("empty"), labels.index("level-error")])
    first = runs[M.CHUNKS[0]][0]
    for chunk, (y, got_codes) in runs.items():
        assert list(got_codes) == list(codes), chunk
        assert not y[codes != M.HG_OK].any()
        for i in ok:
            name = f"chunk {chunk}, request {i} ({labels[i]})"
            assert M.canonical(y[i]), name
            X = M.fe_decode(y[i])
            assert any(c != (0, 0) for c in X), name
            assert X == O.f12_mul(ys[i], O.f12_conj(X)), name
            if labels[i].startswith("zero-"):  # Y = 1: X is its own conjugate
                assert O.f12_is_one(ys[i]) and all(X[k] == (0, 0) for k in (1, 3, 5)), name
    for chunk, (y, _) in runs.items():  # every chunk size right on its own; and then the same words
        _compare(f"fold X, chunk {chunk} against chunk {M.CHUNKS[0]}", y[ok], first[ok],
                 lambda i: f"request {ok[i]} ({labels[ok[i]]})")
    i = labels.index("fourteen-terms")  # n = 1
    y, got_codes = eng.gt_fold(reqs[i:i + 1], words, 8)
    assert list(got_codes) == [0] and (y[0] == first[i]).all()


def test_zero_sum_verdicts_on_the_converted_set(eng):
    """The cross-window zero-sum request through verify_aggregate: the
    aggregate key is infinity; with the signature at infinity and with a real
    signature the codes are the C restatement's."""
    from tests.test_gpu_torus_fold import INFINITY, _want

    ks, reqs, words, labels, _, _ = _fold_case(False)
    _loaded(eng, "torus", ks)
    assert eng.aggregate_tables_torus()
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    pick = [labels.index("zero-two-windows")] * 2 + [labels.index("zero-two-chunks")] * 2 + [labels.index("two-terms")]
    sub = reqs[pick]
    real = R.sign(MSG, (7).to_bytes(32, "big"))
    good = R.sign(MSG, M.fold_scalar(ks, reqs[pick[-1]], words).to_bytes(32, "big"))
    sigs = INFINITY + real + INFINITY + real + good
    want = _want(MSG, reg, sub, words, sigs, eng.flavor_name)
    assert list(eng.verify_aggregate(sub, words, sigs)) == list(want)
    assert want[0] == want[2] and want[1] == want[3] == 1 and want[4] == 0


def test_fold_values_fp12_over_16_key_windows(eng):
    """The same registry with one degenerate pair in window 0: level 2 in Fp12
    form (k_gt_chunks over the 16-key windows): y == conj(g^K), all 120 words."""
    ks = _fold_case(True)[0]
    _loaded(eng, "degenerate", ks)
    assert eng.aggregate_tables() == 2 and not eng.aggregate_tables_torus()
    _check_fp12_fold(eng, True, "fold Y (level 2, Fp12)")


def test_fold_values_over_8_key_windows(eng):
    """Level 1: 28 eight-key windows, up to 28 terms."""
    ks = _fold_case(False)[0]
    _loaded(eng, "level1", ks, level=1)
    assert eng.aggregate_tables() == 1
    eng.set_aggregate_level(1)
    try:
        _check_fp12_fold(eng, False, "fold Y (level 1)")
    finally:
        eng.set_aggregate_level(2)
