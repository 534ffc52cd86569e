"""GPU suite: the two public surfaces that sit directly on the per-thread field
layer (bn256_fp.h be_to_words / fp_from_be, bn256_curve.h g*_mul), against
both CPU oracles (oracle.bn256_oracle and the C restatement oracle.ref_lib).

Non-canonical encodings. A coordinate c < 2^256 - p may travel as c + p:
x/crypto takes coordinates mod p and accepts it, cloudflare refuses it
("coordinate exceeds modulus"). Fixture keys and signatures whose coordinates
all qualify get p added on one coordinate and on all of them; (p, p) and
(p, p, p, p) are NOT infinity (an unmarshal error in go, "exceeds" in cf), and
(p, 0), (0, p) and all-0xFF are invalid too. Every decoding call takes them:
combine, the registry and its aggregate keys, the batch verifiers in both
forms, the per-message verifier, the aggregate verifier on both paths (the
prologue's decode and the pairing kernels' own, every kernel form), and a
store merge. go flavor: codes and bytes equal those of the same call on the
canonical twins and the oracle's; cf flavor: the oracle's error, by the code
tables the suite already uses, the key's before the signature's.

Extreme scalars. keygen, sign and sign_msg on 0, 1, 2, n-1, n, n+1, n+2,
2^255, 2^256-1: multiples of n give all-zero bytes. n and n + 2 are odd, so the
double-and-add ends with an addition of the base point B: for n + 2 to the
accumulator (n + 1) B = B (g*_add's doubling branch), for n to (n - 1) B = -B
(its infinity branch).
"""

import functools

import numpy as np
import pytest

from handel_amd import _lib
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

P = O.P
MSG = F.LIB_MESSAGE
NK = 48
LIMIT = (1 << 256) - P       # c < LIMIT: c + p still fits 32 bytes
CF_PK = {O.ERR_CF_EXCEEDS: _lib.HG_ERR_CF_EXCEEDS, O.ERR_CF_MALFORMED: _lib.HG_ERR_CF_MALFORMED}
CF_SIG = {O.ERR_CF_EXCEEDS: _lib.HG_ERR_SIG_CF_EXCEEDS, O.ERR_CF_MALFORMED: _lib.HG_ERR_SIG_CF_MALFORMED}
FLAVOR_ID = {"go": 0, "cf": 1}


def _coords(m):
    return [int.from_bytes(m[i:i + 32], "big") for i in range(0, len(m), 32)]


def _enc(cs):
    return b"".join(c.to_bytes(32, "big") for c in cs)


def canonical(m):
    """The canonical twin of an encoding x/crypto accepts: every coordinate mod p."""
    return _enc([c % P for c in _coords(m)])


def _variants(m):
    """+p on each single coordinate and on all of them."""
    cs = _coords(m)
    masks = [tuple(i == j for i in range(len(cs))) for j in range(len(cs))] + [(True,) * len(cs)]
    return [_enc([c + P if on else c for c, on in zip(cs, mk)]) for mk in masks]


INVALID_G1 = [_enc([P, P]), _enc([P, 0]), _enc([0, P]), b"\xff" * 64]
INVALID_G2 = [_enc([P, P, P, P]), _enc([P, 0, 0, 0]), _enc([0, 0, 0, P]), b"\xff" * 128]


@functools.lru_cache(maxsize=None)
def corpus():
    """ks, pks, sigs of NK fixture keys on MSG; idx: the keys whose six
    coordinates all lie below 2^256 - p. The conditions the tests rely on are
    asserted here, with the oracle, before any GPU call."""
    ks, pks, sigs = F.keys_and_sigs(NK, MSG, seed=b"encodings")
    pk = [pks[128 * i:128 * i + 128] for i in range(NK)]
    sg = [sigs[64 * i:64 * i + 64] for i in range(NK)]
    idx = [i for i in range(NK) if all(c < LIMIT for c in _coords(pk[i]) + _coords(sg[i]))]
    assert len(idx) >= 3, "three keys with every coordinate below 2^256 - p"
    idx = idx[:3]
    n1 = n2 = 0
    for i in idx:
        for v in _variants(sg[i]):
            pt, err = O.g1_unmarshal(v, "go")
            assert v != sg[i] and canonical(v) == sg[i] and err is None and O.g1_marshal(pt) == sg[i]
            assert O.g1_unmarshal(v, "cf") == (None, O.ERR_CF_EXCEEDS)
            n1 += 1
        for v in _variants(pk[i]):
            pt, err = O.g2_unmarshal(v, "go")
            assert v != pk[i] and canonical(v) == pk[i] and err is None and O.g2_marshal(pt) == pk[i]
            assert O.g2_unmarshal(v, "cf") == (None, O.ERR_CF_EXCEEDS)
            n2 += 1
    assert n1 >= 4 and n2 >= 4  # non-canonical and decoding without error in the go flavor
    for m in INVALID_G1:
        assert O.g1_unmarshal(m, "go")[1] == O.ERR_GO_SIG_UNMARSHAL and O.g1_unmarshal(m, "cf")[1] == O.ERR_CF_EXCEEDS
    for m in INVALID_G2:
        assert O.g2_unmarshal(m, "go")[1] == O.ERR_GO_PK_UNMARSHAL and O.g2_unmarshal(m, "cf")[1] == O.ERR_CF_EXCEEDS
    return ks, pk, sg, idx


@functools.lru_cache(maxsize=None)
def _decode_code(kind, m, flavor):
    """The engine's code of the oracle's decode of one encoding (0: it decodes)."""
    err = (O.g1_unmarshal if kind == "g1" else O.g2_unmarshal)(m, flavor)[1]
    if err is None:
        return 0
    if flavor == "go":
        return _lib.HG_ERR_SIG_UNMARSHAL if kind == "g1" else _lib.HG_ERR_PK_UNMARSHAL
    return (CF_SIG if kind == "g1" else CF_PK)[err]


def _engines(request):
    return [("go", request.getfixturevalue("engine")), ("cf", request.getfixturevalue("engine_cf"))]


# ------------------------------------------------------------------ combine
@pytest.mark.parametrize("kind", ["g1", "g2"])
def test_combine_takes_noncanonical_operands(request, kind):
    ks, pk, sg, idx = corpus()
    src, size, invalid = (sg, 64, INVALID_G1) if kind == "g1" else (pk, 128, INVALID_G2)
    unm, mar, add = (O.g1_unmarshal, O.g1_marshal, O.g1_add) if kind == "g1" else (O.g2_unmarshal, O.g2_marshal, O.g2_add)
    radd = R.g1_add if kind == "g1" else R.g2_add
    a, b = [], []
    for i in idx:
        vs = _variants(src[i])
        other = src[(i + 1) % NK]
        a += vs + [other] * len(vs) + vs + [vs[-1], vs[0]]
        # + another point; the same with the operands swapped; + its canonical self (doubling);
        # + its negation in another encoding (infinity); + itself under another encoding (doubling)
        neg = mar((O.g1_neg if kind == "g1" else O.g2_neg)(unm(src[i])[0]))
        b += [other] * len(vs) + vs + [src[i]] * len(vs) + [neg, vs[-1]]
    a += invalid + [src[0]] * len(invalid) + invalid
    b += [src[1]] * len(invalid) + invalid + invalid[::-1]
    assert len(a) == len(b) <= 64
    for flavor, eng in _engines(request):
        comb = eng.combine_g1 if kind == "g1" else eng.combine_g2
        out, codes = comb(b"".join(a), b"".join(b))
        want_codes = [_decode_code(kind, x, flavor) or _decode_code(kind, y, flavor) for x, y in zip(a, b)]
        assert list(codes) == want_codes, flavor
        if flavor == "cf":
            assert all(want_codes)
            continue
        twin, tcodes = comb(b"".join(canonical(x) if c == 0 else x for x, c in zip(a, want_codes)),
                            b"".join(canonical(y) if c == 0 else y for y, c in zip(b, want_codes)))
        assert list(tcodes) == want_codes
        kinds = set()
        for i, (x, y) in enumerate(zip(a, b)):
            if want_codes[i]:
                continue
            got = out[size * i:size * i + size]
            want = mar(add(unm(x)[0], unm(y)[0]))
            assert got == want == radd(x, y) == twin[size * i:size * i + size], (kind, i)
            kinds.add("infinity" if want == bytes(size) else "doubling" if canonical(x) == canonical(y) else "generic")
        assert kinds == {"infinity", "doubling", "generic"}


# ------------------------------------------------------------------ registry and aggregate keys
def _registry():
    """NK keys, three of them in non-canonical encodings (+p on one coordinate, another, all)."""
    ks, pk, sg, idx = corpus()
    reg = list(pk)
    for j, i in enumerate(idx):
        reg[i] = _variants(pk[i])[(0, 2, 4)[j]]
    return reg


def test_registry_load_and_aggregate_keys(request):
    ks, pk, sg, idx = corpus()
    reg = _registry()
    bad = list(reg[:8]) + INVALID_G2
    ranges = [(0, NK), (idx[0], 1), (idx[1], 1), (min(idx), max(idx) - min(idx) + 1), (0, 16), (16, 32)]
    bitsets = [[True] * s for _, s in ranges]
    bitsets[4] = [i % 3 != 1 for i in range(16)]
    reqs, words = F.pack_requests(ranges, bitsets)
    for flavor, eng in _engines(request):
        from handel_amd.engine import REQ_DTYPE

        assert list(eng.registry_load(b"".join(bad))) == [_decode_code("g2", m, flavor) for m in bad], flavor
        codes = eng.registry_load(b"".join(reg))
        assert list(codes) == [_decode_code("g2", m, flavor) for m in reg], flavor
        if flavor == "cf":
            assert sorted(np.flatnonzero(codes)) == sorted(idx) and set(codes[idx]) == {_lib.HG_ERR_CF_EXCEEDS}
            continue
        agg, acodes = eng.aggregate_pk(np.array(reqs, dtype=REQ_DTYPE), words)
        assert list(acodes) == [0] * len(reqs)
        assert not eng.registry_load(b"".join(pk)).any()
        twin, tcodes = eng.aggregate_pk(np.array(reqs, dtype=REQ_DTYPE), words)
        assert agg == twin and list(tcodes) == [0] * len(reqs)
        for r, ((off, size), bits) in enumerate(zip(ranges, bitsets)):
            kind, want = O.aggregate_pk([O.g2_unmarshal(m, "go")[0] for m in reg[off:off + size]], bits)
            got = agg[128 * r:128 * r + 128]
            assert kind == "ok" and got == O.g2_marshal(want) and all(c < P for c in _coords(got)), r  # the canonical marshal


# ------------------------------------------------------------------ the batch verifiers
@functools.lru_cache(maxsize=None)
def _checks():
    """(pk, sig) pairs on MSG over the variants, wrong keys and the invalid encodings."""
    ks, pk, sg, idx = corpus()
    cs = []
    for pos, i in enumerate(idx):
        cs += [(pk[i], v) for v in _variants(sg[i])]
        cs += [(v, sg[i]) for v in _variants(pk[i])]
        cs += [(_variants(pk[i])[-1], _variants(sg[i])[-1]),                        # both non-canonical
               (_variants(pk[i])[0], _variants(sg[idx[(pos + 1) % len(idx)]])[1]),  # and another key's signature
               (pk[i], sg[i])]
    cs += [(pk[0], m) for m in INVALID_G1] + [(m, sg[0]) for m in INVALID_G2]
    cs += [(INVALID_G2[0], INVALID_G1[0]), (INVALID_G2[3], _variants(sg[idx[0]])[0])]  # the key's error comes first
    assert len(cs) <= 64
    return cs


def _want_codes(cs, flavor, msgs=None):
    want = []
    for k, (p, s) in enumerate(cs):
        c = _decode_code("g2", p, flavor) or _decode_code("g1", s, flavor)
        if c == 0:
            c = int(R.verify_batch(msgs[k] if msgs else MSG, p, s, flavor=FLAVOR_ID[flavor])[0])
            assert c in (0, 1)
        want.append(c)
    return want


def _fold(codes):
    """The engine's cloudflare codes in the C oracle's terms (one code per unmarshal failure: 4 pk, 5 sig)."""
    return [4 if 7 <= c <= 9 else 5 if 10 <= c <= 12 else int(c) for c in codes]


@pytest.mark.parametrize("split", [False, True], ids=["one_kernel", "split"])
def test_verify_batch_takes_noncanonical_encodings(request, split):
    cs = _checks()
    pks, sigs = b"".join(p for p, _ in cs), b"".join(s for _, s in cs)
    for flavor, eng in _engines(request):
        want = _want_codes(cs, flavor)
        assert _fold(want) == list(R.verify_batch(MSG, pks, sigs, flavor=FLAVOR_ID[flavor]))  # the two oracles agree
        assert eng.set_message(MSG) == 0
        eng.set_verify_split(split)
        try:
            got = eng.verify_batch(pks, sigs)
            twin = eng.verify_batch(b"".join(canonical(p) if c in (0, 1) else p for (p, _), c in zip(cs, want)),
                                    b"".join(canonical(s) if c in (0, 1) else s for (_, s), c in zip(cs, want)))
        finally:
            eng.set_verify_split(False)
        assert list(got) == want, flavor
        if flavor == "go":
            assert list(twin) == want
            assert want.count(0) >= 20 and want.count(1) >= 3 and want.count(4) >= 5 and want.count(5) >= 4
        else:
            assert want.count(0) == 3 and want.count(_lib.HG_ERR_CF_EXCEEDS) >= 20 \
                and want.count(_lib.HG_ERR_SIG_CF_EXCEEDS) >= 10


def test_verify_batch_msgs_takes_noncanonical_encodings(request):
    ks, pk, sg, idx = corpus()
    other = F.TEST_MESSAGES[0]
    cs = list(_checks()) + [(pk[5], R.sign(other, ks[5].to_bytes(32, "big"))), (pk[6], sg[6])]
    msgs = [MSG] * len(_checks()) + [other, other]
    pks, sigs = b"".join(p for p, _ in cs), b"".join(s for _, s in cs)
    for flavor, eng in _engines(request):
        want = _want_codes(cs, flavor, msgs)
        assert want[-2:] == [0, 1]
        assert list(eng.verify_batch_msgs(msgs, pks, sigs)) == want, flavor
        if flavor == "go":
            twin = eng.verify_batch_msgs(msgs, b"".join(canonical(p) if c in (0, 1) else p for (p, _), c in zip(cs, want)),
                                         b"".join(canonical(s) if c in (0, 1) else s for (_, s), c in zip(cs, want)))
            assert list(twin) == want


# ------------------------------------------------------------------ the aggregate verifier
@functools.lru_cache(maxsize=None)
def _aggregate_batch():
    """Requests over the NK-key registry whose aggregate signatures have both
    coordinates below 2^256 - p, each in its canonical form, with +p on x, on y
    and on both, one of them tampered; then the invalid encodings."""
    ks, pk, sg, idx = corpus()
    rng = np.random.default_rng(20241021)
    ranges, bitsets, sigs = [], [], []
    cands = [(0, NK), (0, 16), (16, 16), (32, 16), (8, 8), (idx[0], 1), (3, 20)]
    picked = 0
    for off, size in cands * 3:
        if picked == 4:
            break
        bits = [bool(b) for b in rng.random(size) < 0.7]
        bits[0] = True
        k = sum(ks[off + i] for i, b in enumerate(bits) if b) % O.ORDER
        s = R.sign(MSG, k.to_bytes(32, "big"))
        if not all(c < LIMIT for c in _coords(s)):
            continue
        picked += 1
        vs = [s] + _variants(s)
        if picked == 2:  # a wrong aggregate in every encoding
            t = F.tamper(s, every=1)
            while not all(c < LIMIT for c in _coords(t)):
                t = F.tamper(t, every=1)
            vs = [t] + _variants(t)
        for v in vs:
            ranges.append((off, size))
            bitsets.append(bits)
            sigs.append(v)
    assert picked == 4
    for m in INVALID_G1:
        ranges.append((0, 16))
        bitsets.append([True] * 16)
        sigs.append(m)
    ranges.append((4, 9))          # an empty set with a non-canonical signature
    bitsets.append([False] * 9)
    sigs.append(sigs[1])
    assert len(sigs) <= 64
    return ranges, bitsets, sigs


def test_verify_aggregate_takes_noncanonical_encodings(request, agg_level):
    from handel_amd.engine import REQ_DTYPE

    ks, pk, sg, idx = corpus()
    ranges, bitsets, sigs = _aggregate_batch()
    rq, words = F.pack_requests(ranges, bitsets)
    reqs = np.array(rq, dtype=REQ_DTYPE)
    sigb = b"".join(sigs)
    for flavor, eng in _engines(request):
        reg = b"".join(_registry() if flavor == "go" else pk)  # cloudflare refuses the non-canonical keys at load
        want, want_agg = R.verify_aggregate(MSG, reg, reqs["offset"], reqs["bitlen"], reqs["level_size"], words,
                                            reqs["word_offset"].astype(np.uint64), sigb, nthreads=8, want_agg=True)
        want = [int(c) for c in want]
        for i, s in enumerate(sigs):
            # the Python oracle's decode. go: the restatement's verdict; cf: the restatement decodes
            # as go, and a signature's decode error comes before every other code of its request
            c = _decode_code("g1", s, flavor)
            if flavor == "go":
                assert (c != 0) == (want[i] == _lib.HG_ERR_SIG_UNMARSHAL), i
            want[i] = c or want[i]
        assert not eng.registry_load(reg).any() and eng.set_message(MSG) == 0
        codes, agg = eng.verify_aggregate(reqs, words, sigb, want_agg=True)
        assert list(codes) == want, (flavor, agg_level)
        assert list(eng.verify_aggregate(reqs, words, sigb)) == want, (flavor, agg_level)
        for i, c in enumerate(want):
            if c in (0, 1):
                assert agg[128 * i:128 * i + 128] == want_agg[128 * i:128 * i + 128], (flavor, i)
        if flavor == "go":
            assert want.count(0) >= 10 and want.count(1) >= 1 and want.count(_lib.HG_ERR_SIG_UNMARSHAL) == 4
            assert want[-1] == _lib.HG_ERR_EMPTY_AGG
            assert not eng.registry_load(b"".join(pk)).any()
            twin = eng.verify_aggregate(reqs, words, b"".join(canonical(s) if c in (0, 1, 6) else s
                                                              for s, c in zip(sigs, want)))
            assert list(twin) == want
        else:
            assert want.count(0) == 3 and want.count(_lib.HG_ERR_SIG_CF_EXCEEDS) >= 14


def test_every_pairing_kernel_decodes_noncanonical_signatures(engine):
    """The GT path's pairing kernels decode their own signatures
    (hg_sig_pairing_device's five forms): the FE bytes of a non-canonical
    encoding are those of its canonical twin."""
    import torch

    import bench

    ks, pk, sg, idx = corpus()
    sigs = [v for i in idx for v in _variants(sg[i])] + [sg[0], bytes(64)]
    n = len(sigs)
    dev = torch.device("cuda", 0)
    assert engine.set_message(MSG) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = {}
    for name, batch in (("given", sigs), ("twin", [canonical(s) for s in sigs])):
        d_sigs = bench._dev_bytes(b"".join(batch), dev)
        for k in range(5):
            fe = torch.full((n * 480,), 0x5A, dtype=torch.uint8, device=dev)
            engine.sig_pairing_device(d_sigs.data_ptr(), n, fe.data_ptr(), k, stream)
            torch.cuda.synchronize(dev)
            outs[name, k] = fe.cpu().numpy().reshape(n, 480)
    for k in range(5):
        bad = np.flatnonzero((outs["given", k] != outs["twin", k]).any(axis=1))
        assert bad.size == 0, f"kernel {k}: signatures {bad.tolist()} differ from their canonical twins"
        assert np.array_equal(outs["twin", k], outs["twin", 0]), k
    assert not np.array_equal(outs["twin", 0][0], outs["twin", 0][3])  # different signatures, different values


# ------------------------------------------------------------------ one store merge
def test_store_merge_of_a_noncanonical_signature():
    """An entry whose signature is a non-canonical encoding stores the row
    bytes of its canonical twin: as a first best, merged with a disjoint best,
    and doubled with itself under another encoding. (go flavor: a cloudflare
    verifier never passes such a signature on to the store.)"""
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import Store
    from tests import test_gpu_store_merge as M

    ks, pk, sg, idx = corpus()
    nreg = 64
    e = M._engine(nreg, "go")
    try:
        i, j = idx[0], idx[1]
        vi, vj = _variants(sg[i]), _variants(sg[j])
        host = {5: Store(5, nreg, M._oracle_combine)}
        st = DeviceStores(e, [5], 8)
        st.enable_merge()
        given = [M.Entry(5, 6, 40, 0b0011, vi[2]), M.Entry(5, 6, 42, 0b1100, vj[0]),    # first best, then a disjoint merge
                 M.Entry(5, 5, 20, 0b0001, vi[0]), M.Entry(5, 5, 21, 0b0110, vi[1]),    # the same point twice: doubling
                 M.Entry(5, 4, 9, 0b01, vj[2])]                                         # a first best alone
        twins = [M.Entry(en.receiver, en.level, en.origin, en.bits, canonical(en.sig)) for en in given]
        want = M._host_apply(host, nreg, twins)
        assert want[0] == [M.STORED] * 5
        assert M._run_merge(e, st, nreg, given) == want
        M._assert_rows_equal(st, host, nreg)
        assert st.read_best(5, 6)[1] == O.g1_marshal(O.g1_add(O.g1_unmarshal(sg[i])[0], O.g1_unmarshal(sg[j])[0]))
        assert st.read_best(5, 5)[1] == R.g1_add(sg[i], sg[i]) and st.read_best(5, 4)[1] == sg[j]
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ extreme scalars
N = O.ORDER
SCALARS = [0, 1, 2, N - 1, N, N + 1, N + 2, 1 << 255, (1 << 256) - 1]


def test_keygen_and_sign_on_extreme_scalars(request):
    sb = F.scalar_bytes(SCALARS)
    h = O.hashed_message(MSG)[0]
    other = F.TEST_MESSAGES[1]
    h2 = O.hashed_message(other)[0]
    want_pk = b"".join(O.g2_marshal(O.g2_mul(O.G2_GEN, k)) for k in SCALARS)
    want_sig = b"".join(O.g1_marshal(O.g1_mul(h, k)) for k in SCALARS)
    want_sig2 = b"".join(O.g1_marshal(O.g1_mul(h2, k)) for k in SCALARS)
    assert want_pk == R.g2_scalar_base(sb) and want_sig == R.sign(MSG, sb) and want_sig2 == R.sign(other, sb)
    for k, name in ((0, "0"), (4, "n")):  # multiples of n: all-zero bytes
        assert want_pk[128 * k:128 * k + 128] == bytes(128) and want_sig[64 * k:64 * k + 64] == bytes(64), name
    assert want_pk[128 * 5:128 * 6] == want_pk[128:256] == O.g2_marshal(O.G2_GEN)  # n + 1
    assert want_sig[64 * 6:64 * 7] == want_sig[128:192]                            # n + 2 is 2: the doubling branch
    for flavor, eng in _engines(request):
        assert eng.keygen(sb) == want_pk, flavor
        assert eng.set_message(MSG) == 0
        assert eng.sign(sb) == want_sig, flavor
        assert eng.sign_msg(other, sb) == want_sig2, flavor
        assert eng.sign_msg(MSG, sb) == want_sig, flavor
