"""CPU model of the speculative segment-parallel chain of cmx_mixnet_spec_kernel (cmix_amd/csrc/mixnet_chunk.hip, helper_role): which path
the resolve of every speculative segment takes. A plain helper module of tests/test_spec_model.py (CPU) and tests/test_gpu_spec_chain.py (GPU).

The arithmetic is oracle/spec_probe.c (built into the oracle's library): it sees the inputs and the selected row of every layer-0 Mix of an
oracle run through the orc_mix_probe hook, forms the rounded products, the f32 running sum at elements 512, 1024 and 1536 (the true starts),
the f64 estimate exactly as the kernel's waves form it, and offset = f2ord(true start) - f2ord((float)estimate). A segment is a HIT when
-32 <= offset <= 31 (through lane offset + 32: the kernel's 64 candidates are ord2f(f2ord((float)est) + lane - 32)), else a re-run.

This module adds the bookkeeping (counts in the form of MixNet.spec_stats()), the shared 512-bit stream, and the crafted rows: single bits
whose layer-0 row of one mixer is built by weight injection so that one named resolve path is taken (binade crossings, zero crossings in
the subnormals, terms at the segment seams and in the last wave's tail)."""
import ctypes as C
import functools

import numpy as np

from conftest import synth_mixnet_inputs

N_IN0, N_MIX, N_MIX0, SEG = 2078, 47, 26, 512
AUX_MIXER = 12          # its selector key comes out of the inputs (predictor.cpp:388-393): never crafted

REC = np.dtype([("offset", "<i8", 3), ("start", "<u4", 3), ("centre", "<u4", 3), ("resolved", "<u4", 3), ("serial", "<u4", 3),
                ("sum", "<u4"), ("pad", "<u4")])
assert REC.itemsize == 80


def _lib():
    from oracle import oracle as O
    L = O.lib()
    L.orc_spec_model.argtypes = [C.c_void_p, C.c_void_p]
    L.orc_spec_record_begin.argtypes = [C.c_void_p, C.c_size_t]
    L.orc_spec_record_end.restype = C.c_size_t
    return L


def f2ord(bits):
    """the kernel's f2ord on bit patterns (uint32 array) -> int64: consecutive floats are consecutive integers, -0.0 -> -1, +0.0 -> 0"""
    b = np.asarray(bits, np.uint32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7fffffff, b)


def from_products(prod):
    """the model on one vector of 2078 rounded products -> one REC record"""
    prod = np.ascontiguousarray(prod, np.float32)
    assert prod.shape == (N_IN0,)
    out = np.zeros(1, REC)
    _lib().orc_spec_model(prod.ctypes.data, out.ctypes.data)
    return out[0]


def run(probs, sel, bits, inject=()):
    """An oracle run over the stream with the model attached. inject: (mixer, key, index, float32 value) set before the first bit.
    -> p [T] f32, mix_out [T,47] f32, records [T,26] REC"""
    from oracle import oracle as O
    L = _lib()
    T = len(bits)
    net = O.MixNet()
    for mixer, key, index, value in inject:
        net.set_weight(mixer, key, index, value)
    recs = np.zeros(T * N_MIX0, REC)
    p = np.empty(T, np.float32)
    mix = np.empty((T, N_MIX), np.float32)
    L.orc_spec_record_begin(recs.ctypes.data, len(recs))
    try:
        for t in range(T):
            p[t], mix[t] = net.step(probs[t], sel[t], bits[t], want_mix=True)
    finally:
        n = L.orc_spec_record_end()
    net.close()
    assert n == len(recs), "the probe saw %d layer-0 mixes, %d expected" % (n, len(recs))
    return p, mix, recs.reshape(T, N_MIX0)


def is_hit(recs):
    """[..., 3] bool: segment 1..3 resolves from a candidate lane"""
    return (recs["offset"] >= -32) & (recs["offset"] <= 31)


def counts(recs):
    """what MixNet.spec_stats() must report after exactly these mixes"""
    hit = is_hit(recs).reshape(-1, 3)
    return {"segments": int(hit.size), "hits": int(hit.sum()), "reruns": [int(x) for x in (~hit).sum(axis=0)]}


def stats_of(spec_stats):
    """MixNet.spec_stats() in the form of counts()"""
    return {"segments": int(spec_stats["segments"]), "hits": int(spec_stats["hits"]), "reruns": [int(x) for x in spec_stats["reruns"]]}


SYNTH_T, SYNTH_SEED = 512, 11


@functools.lru_cache(maxsize=None)
def synthetic():
    """The shared 512-bit stream: inputs, the oracle's p and mixer outputs, the model's records. Computed once; read-only."""
    probs, sel, bits = synth_mixnet_inputs(SYNTH_T, seed=SYNTH_SEED)
    p, mix, recs = run(probs, sel, bits)
    for a in (probs, sel, bits, p, mix, recs):
        a.setflags(write=False)
    return {"probs": probs, "sel": sel, "bits": bits, "p": p, "mix": mix, "recs": recs}


# ---------------------------------------------------------------------------------------------------------------- crafted rows
# Every crafted bit has all 2078 inputs at CRAFT_P and a selector key of its own on every mixer (bit c: key c), so every mixer selects a
# fresh all-zero row; one mixer's row gets the case's weights by injection before the stream starts. A fresh row's extra weights are zero,
# so that mixer's output IS the ordered sum of the 2078 products. On the device a mixer's rows are numbered in order of first touch
# (select_row, mixnet_dev.h): key c of bit c is row c -- except on the auxiliary-context mixer, whose key the inputs decide.
CRAFT_P = np.float32(0.75)
N_CRAFTED = 35          # len(crafted_cases()), known without building them


def _f32(v):
    return np.float32(v)


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _step(w, n):
    """the float n steps above (n > 0) / below w in the ordered-integer image"""
    o = int(f2ord(np.array([_bits(w)], np.uint32))[0]) + n
    b = (o ^ 0x7fffffff) if o < 0 else o
    return np.array([b & 0xffffffff], np.uint32).view(np.float32)[0]


def _weight_for(x, accept, w0):
    """a weight near w0 whose rounded product with x satisfies accept(product)"""
    for n in sorted(range(-64, 65), key=abs):
        w = _step(_f32(w0), n)
        if accept(_f32(x * w)):
            return w
    raise AssertionError("no weight near %r gives the wanted product" % (w0,))


class Case:
    def __init__(self, name, weights, segment=None, claim=None):
        self.name, self.weights, self.segment, self.claim = name, weights, segment, claim
        self.bit = self.mixer = None   # placed by crafted_cases()

    def __repr__(self):
        return "Case(%s)" % self.name


def _binade_case(x, q, below, miss):
    """Segment q's true start and candidate centre in different binades. below: the true start just below 1.0 and the centre above it
    (one product just under 1.0, then products of a quarter ulp each, which the f32 chain drops one by one and the f64 estimate keeps);
    else the true start at / just above 1.0 and the centre below it (negative products of an eighth of the ulp above 1.0)."""
    one = _f32(1.0)
    w = {}
    if below:
        w[0] = _weight_for(x, lambda p: p < one and p >= _step(one, -3), one / x)
        tiny = _f32(2.0 ** -26)
    else:
        w[0] = _weight_for(x, lambda p: p >= one and p <= _step(one, 1), one / x)
        tiny = _f32(-(2.0 ** -26))
    wt = _f32(tiny / x)
    pt = abs(_f32(x * wt))
    assert 2.0 ** -27 < pt < 2.0 ** -25
    n = 400 if miss else 32
    for i in range(n):
        w[SEG * (q - 1) + 1 + i] = wt
    name = "binade seg %d: true start %s 1.0, centre %s, %s" % (q, "below" if below else "at or above", "above" if below else "below", "miss" if miss else "hit")
    return Case(name, w, q, ("binade", "miss" if miss else "hit", below))


def _edge_case(x, q, offset):
    """Segment q's true start exactly `offset` candidates from the centre (the window is -32..+31): B ~ 1.1, then |offset| * 8 products of an
    eighth of B's ulp, of the opposite sign, which the f32 chain drops and the f64 estimate keeps."""
    w = {0: _f32(1.0)}
    wt = _f32((-1 if offset > 0 else 1) * 2.0 ** -26 / x)
    for i in range(8 * abs(offset)):
        w[SEG * (q - 1) + 1 + i] = wt
    return Case("edge seg %d: offset %+d" % (q, offset), w, q, ("edge", offset))


def _sub(units):
    return np.array([(abs(units) | (0x80000000 if units < 0 else 0))], np.uint32).view(np.float32)[0]


def _zero_case(x, q, dropped, kept):
    """Segment q's candidate window across zero, in the f32 subnormals (units of 2^-149). Products, in chain order: B ~ 1 (element b, lane 0),
    `dropped` units (element b + 1: B + it rounds back to B), -B (element b + 64: lane 0 again, so lane 0's f64 partial sum is exactly 0 and
    the f32 chain is exactly +0.0 after it), `kept` units (element b + 65, if not 0). True start: `kept` units; centre: dropped + kept units."""
    b = SEG * (q - 1)
    w = {b: _f32(1.0)}
    w[b + 64] = _f32(-1.0)

    def sub_weight(units):
        for m in range(1, 64):
            c = _sub(m if units > 0 else -m)
            if _bits(_f32(x * c)) == _bits(_sub(units)):
                return c
        raise AssertionError("no subnormal weight gives %d units" % units)
    w[b + 1] = sub_weight(dropped)
    if kept:
        w[b + 65] = sub_weight(kept)
    name = "zero seg %d: true start %+d units of 2^-149, centre %+d units" % (q, kept, dropped + kept)
    return Case(name, w, q, ("zero", kept, dropped + kept))


def _triple(x, at):
    """a non-associative triple (big, -big, small) at elements at, at + 1, at + 2: (big + -big) + small = small, any other order or a dropped term differs"""
    return {at: _f32(2.0 ** 24), at + 1: _f32(-(2.0 ** 24)), at + 2: _f32(0.25)}


@functools.lru_cache(maxsize=None)
def crafted_cases():
    from oracle import oracle as O
    x = O.stretch(CRAFT_P)
    assert 1.0 < x < 1.2
    cases = []
    for q in (1, 2, 3):
        for below in (True, False):
            for miss in (False, True):
                cases.append(_binade_case(x, q, below, miss))
    for q, offs in ((1, (-33, -32, 31, 32)), (2, (-32, 31)), (3, (-32, 31))):   # lane 0 and lane 63, and the first miss on either side
        for o in offs:
            cases.append(_edge_case(x, q, o))
    for q in (1, 2, 3):
        cases.append(_zero_case(x, q, -5, 0))     # true start +0.0, negative subnormal centre: a hit six lanes above the centre
        cases.append(_zero_case(x, q, -10, 3))    # positive subnormal true start, negative centre
        cases.append(_zero_case(x, q, 10, -3))    # the mirror image
    for s in (512, 1024, 1536, 2048):
        cases.append(Case("seam %d: (big, -big, small) at %d, %d, %d" % (s, s - 1, s, s + 1), _triple(x, s - 1), None, ("seam", s)))
    tail = _triple(x, 2048)   # then 27 distinct terms of the small one's size, each of which moves the sum
    for i in range(3, 30):
        tail[2048 + i] = _f32(0.25 + i * 2.0 ** -6 + 2.0 ** -20)
    cases.append(Case("tail: (big, -big, small) and 27 distinct terms at 2048..2077", tail, None, ("tail", 30)))
    cases.append(Case("tail: element 2077 alone", {2077: _f32(0.25)}, None, ("tail", 1)))
    mixers = [m for m in range(N_MIX0) if m != AUX_MIXER]
    for c, case in enumerate(cases):
        case.bit, case.mixer = c, mixers[c % len(mixers)]
    assert len(cases) == N_CRAFTED
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def crafted():
    """The crafted stream (one case per bit), the oracle's p and mixer outputs with the same injection, the model's records. Read-only."""
    cases = crafted_cases()
    T = len(cases)
    probs = np.full((T, N_IN0), CRAFT_P, np.float32)
    sel = np.repeat(np.arange(T, dtype=np.uint64)[:, None], N_MIX, axis=1)
    bits = (np.arange(T) % 2).astype(np.uint8)
    inject = [(c.mixer, c.bit, i, v) for c in cases for i, v in sorted(c.weights.items())]
    p, mix, recs = run(probs, sel, bits, inject)
    for a in (probs, sel, bits, p, mix, recs):
        a.setflags(write=False)
    return {"cases": cases, "probs": probs, "sel": sel, "bits": bits, "p": p, "mix": mix, "recs": recs}


def exponent(bits):
    return (np.asarray(bits, np.uint32) >> 23) & 0xff
