"""CPU model (numpy) of the split re-run of cmx_mixnet_spec_kernel's speculative chain (cmix_amd/csrc/mixnet_chunk.hip, helper_role's miss
branch). A plain helper module of tests/test_spec_rerun_model.py (CPU) and tests/test_gpu_spec_rerun.py (GPU); it builds on tests/spec_model.py.

A segment q = 1..3 whose true start lies outside the 64 start candidates is re-run from the true start s. The re-run is itself speculative
inside its wave: lane 0 adds the segment's first 256 products to s, lanes 1..63 add the remaining products (256, the last segment 286) to the
63 floats ord2f(f2ord((float)mid_est) + lane - 32), where mid_est = (double)s + the wave sum of the per-lane f64 sums of the first 256
products (lane l: 0.0 + p[l] + p[64 + l] + p[128 + l] + p[192 + l], then wave_sum_f64's tree). If a candidate lane has the true mid-point's
bit pattern the re-run resolves there (a MID HIT: offset of the true mid-point from the centre in -31..+31), else the second half runs
serially from the true mid-point (a SERIAL HALF). The model restates this operation for operation on one vector of 2078 rounded products and
says which of the two every missed segment takes; the start offsets it forms on the way must equal spec_model.from_products'.

The products come through the oracle's orc_mix_probe hook, installed from Python (run()); the crafted rows extend spec_model's by rows that
miss at a segment's start AND put the mid-point where a named path is taken."""
import ctypes as C
import functools

import numpy as np

import spec_model as S

N_IN0, N_MIX, N_MIX0, SEG, HALF = S.N_IN0, S.N_MIX, S.N_MIX0, S.SEG, S.SEG // 2
MID_LO, MID_HI = -31, 31          # lanes 1..63: lane j starts from centre + j - 32
N_CRAFTED = 41                    # len(crafted_cases()), known without building them

RR = np.dtype([("start_offset", "<i8", 3), ("miss", "?", 3), ("mid_offset", "<i8", 3), ("mid_hit", "?", 3),
               ("mid", "<u4", 3), ("mid_centre", "<u4", 3)])


def wave_sum(v):
    """wave_sum_f64 as the lanes that are read see it: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:4, row_ror:8, then
    (lane 0 + lane 16) + (lane 32 + lane 48)"""
    v = np.asarray(v, np.float64).reshape(4, 4, 4)          # row of 16, quad, lane of the quad
    q = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
    r = (q[:, 0] + q[:, 3]) + (q[:, 2] + q[:, 1])           # lane 0 reads lane 12, lane 8 reads lane 4, lane 0 reads lane 8
    return (r[0] + r[1]) + (r[2] + r[3])


def _lane_sums(p, n):
    """per lane: 0.0 + p[l] + p[64 + l] + ... (n terms), in f64, in this order"""
    ds = np.zeros(64, np.float64)
    for k in range(n):
        ds = ds + p[64 * k:64 * k + 64].astype(np.float64)
    return ds


def model(prod):
    """the split re-run on one vector of 2078 rounded products -> one RR record"""
    prod = np.ascontiguousarray(prod, np.float32)
    assert prod.shape == (N_IN0,)
    run = np.cumsum(np.concatenate([np.zeros(1, np.float32), prod]), dtype=np.float32)   # run[i]: 0.0f + p[0] + ... + p[i - 1], sequentially rounded
    out = np.zeros(1, RR)[0]
    est = np.float64(0.0)
    for q in (1, 2, 3):
        est = est + wave_sum(_lane_sums(prod[SEG * (q - 1):SEG * q], 8))
        s = run[SEG * q]
        off = int(S.f2ord(s.view(np.uint32)) - S.f2ord(np.float32(est).view(np.uint32)))
        out["start_offset"][q - 1] = off
        miss = not (-32 <= off <= 31)
        out["miss"][q - 1] = miss
        mid_est = np.float64(s) + wave_sum(_lane_sums(prod[SEG * q:SEG * q + HALF], 4))
        centre = np.float32(mid_est)
        mid = run[SEG * q + HALF]
        moff = int(S.f2ord(mid.view(np.uint32)) - S.f2ord(centre.view(np.uint32)))
        out["mid_offset"][q - 1] = moff
        out["mid_hit"][q - 1] = MID_LO <= moff <= MID_HI
        out["mid"][q - 1] = mid.view(np.uint32)
        out["mid_centre"][q - 1] = centre.view(np.uint32)
    return out


def counts(rr):
    """what MixNet.spec_rerun_stats() must report after exactly these mixes"""
    miss, hit = rr["miss"].reshape(-1, 3), rr["mid_hit"].reshape(-1, 3)
    return {"mid_hits": int((miss & hit).sum()), "serial_halves": int((miss & ~hit).sum())}


def paths(rr):
    """per segment 1..3: (mid hits, serial halves) among the missed segments"""
    miss, hit = rr["miss"].reshape(-1, 3), rr["mid_hit"].reshape(-1, 3)
    return [(int((miss & hit)[:, q].sum()), int((miss & ~hit)[:, q].sum())) for q in range(3)]


_PROBE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int)


def run(probs, sel, bits, inject=()):
    """An oracle run over the stream with a Python probe on orc_mix_probe: the rounded products of every layer-0 Mix go through
    spec_model.from_products and model(). -> p [T], mix [T,47], records [T,26] REC, re-run records [T,26] RR"""
    from oracle import oracle as O
    L = O.lib()
    T = len(bits)
    recs, rrs = [], []

    def probe(_mixer, x, w, n):
        if n != N_IN0:
            return
        prod = np.ctypeslib.as_array(x, (n,)) * np.ctypeslib.as_array(w, (n,))      # float32 * float32, rounded (mixer.cpp:41)
        recs.append(S.from_products(prod))
        rrs.append(model(prod))
    cb = _PROBE(probe)
    hook = C.c_void_p.in_dll(L, "orc_mix_probe")
    net = O.MixNet()
    for mixer, key, index, value in inject:
        net.set_weight(mixer, key, index, value)
    p = np.empty(T, np.float32)
    mix = np.empty((T, N_MIX), np.float32)
    hook.value = C.cast(cb, C.c_void_p).value
    try:
        for t in range(T):
            p[t], mix[t] = net.step(probs[t], sel[t], bits[t], want_mix=True)
    finally:
        hook.value = None
    net.close()
    assert len(recs) == T * N_MIX0, "the probe saw %d layer-0 mixes, %d expected" % (len(recs), T * N_MIX0)
    return p, mix, np.array(recs, S.REC).reshape(T, N_MIX0), np.array(rrs, RR).reshape(T, N_MIX0)


@functools.lru_cache(maxsize=None)
def synthetic():
    """spec_model's shared 512-bit stream once more, with the re-run records. Computed once; read-only."""
    d = S.synthetic()
    p, mix, recs, rr = run(d["probs"], d["sel"], d["bits"])
    assert np.array_equal(p.view(np.uint32), d["p"].view(np.uint32)) and np.array_equal(mix.view(np.uint32), d["mix"].view(np.uint32))
    for a in (recs, rr):
        a.setflags(write=False)
    return {"recs": recs, "rr": rr}


# ---------------------------------------------------------------------------------------------------------------- crafted rows
# As spec_model's: every input at CRAFT_P (x = stretch(0.75) ~ 1.0986), a fresh row per bit, one mixer's row injected. Every case here MISSES at
# the start of a segment q (so the re-run runs) and places the true mid-point of q relative to its estimate. Terms the f32 chain drops and
# the f64 estimates keep: an eighth of B's ulp (2^-26, spec_model's, in segment q - 1: they move the START estimate) and a quarter of it
# (2^-25, in the first half of segment q: 255 places, so up to 63 ulps; anything under half an ulp is dropped by the chain).
def _start_miss(x, q, offset):
    """spec_model's edge row: B = x at element 0, 8 |offset| dropped eighths in segment q - 1 -> start offset `offset` for q (and every later segment)"""
    return dict(S._edge_case(x, q, offset).weights)


def _mid_terms(x, q, offset):
    """|offset| * 4 dropped quarters of B's ulp at the head of segment q (after its first term's place): the true mid-point `offset` from its estimate"""
    n = 4 * abs(offset)
    assert n <= HALF - 1
    wt = S._f32((-1 if offset > 0 else 1) * 2.0 ** -25 / x)
    return {SEG * q + 1 + i: wt for i in range(n)}


def _sub_weight(x, units):
    for m in range(1, 64):
        c = S._sub(m if units > 0 else -m)
        if S._bits(S._f32(x * c)) == S._bits(S._sub(units)):
            return c
    raise AssertionError("no subnormal weight gives %d units" % units)


def _zero_mid(x, q, dropped, kept):
    """The mid-point window across zero, in the subnormals. Segment q - 1: B, 320 dropped eighths, -B (lane 0 both): the true start is +0.0 and the
    start estimate 40 ulps of B away, a miss. Segment q, first half: B (element b), `dropped` units of 2^-149 (b + 1: B + it is B), -B (b + 64: lane 0
    again, exact in f64 and f32), `kept` units (b + 65). True mid-point: `kept` units; centre: dropped + kept units."""
    a, b = SEG * (q - 1), SEG * q
    w = {a: S._f32(1.0), a + 384: S._f32(-1.0)}
    wt = S._f32(-(2.0 ** -26) / x)
    for i in range(320):
        w[a + 1 + i] = wt
    w[b], w[b + 64] = S._f32(1.0), S._f32(-1.0)
    w[b + 1] = _sub_weight(x, dropped)
    if kept:
        w[b + 65] = _sub_weight(x, kept)
    return w


def _binade_mid(x, q, below):
    """The mid-point and its centre in different binades: spec_model's binade row that misses at the start of q (one product next to 1.0, 400 dropped
    quarter-ulp terms in segment q - 1), and 32 more of the same terms at the head of segment q: the chain stays where it is, the estimate crosses 1.0."""
    w = dict(S._binade_case(x, q, below, True).weights)
    wt = w[SEG * (q - 1) + 1]
    for i in range(32):
        w[SEG * q + 1 + i] = wt
    return w


def _tail_terms():
    return {2048 + i: S._f32(0.25 + i * 2.0 ** -6 + 2.0 ** -20) for i in range(30)}


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """-> tuple of spec_model.Case; claim = {segment: ("mid", offset) | ("serial", offset)}: the mid-point path the case is built for"""
    from oracle import oracle as O
    x = O.stretch(S.CRAFT_P)
    cases = []

    def add(name, w, claim):
        cases.append(S.Case(name, w, None, claim))
    for q in (1, 2, 3):                                    # (a) a start miss on either side, the mid-point on its estimate
        for so in (40, -40):
            add("(a) seg %d: start %+d, mid-point at 0" % (q, so), _start_miss(x, q, so), {q: ("mid", 0)})
    for q, offs in ((1, (-33, -32, -31, 30, 31, 32)), (2, (-32, -31, 31, 32)), (3, (-32, -31, 31, 32))):   # (b) the window's edge lanes 1 and 63, and outside
        for mo in offs:
            w = _start_miss(x, q, 40)
            w.update(_mid_terms(x, q, mo))
            add("(b) seg %d: mid-point at %+d" % (q, mo), w, {q: ("mid" if MID_LO <= mo <= MID_HI else "serial", mo)})
    for q in (1, 2, 3):                                    # (c) across zero in the subnormals (f2ord(-k units) = -k - 1), across a binade
        add("(c) seg %d: mid-point +0.0, centre -5 units" % q, _zero_mid(x, q, -5, 0), {q: ("mid", 6)})
        add("(c) seg %d: mid-point +3 units, centre -7 units" % q, _zero_mid(x, q, -10, 3), {q: ("mid", 11)})
        add("(c) seg %d: mid-point -3 units, centre +7 units" % q, _zero_mid(x, q, 10, -3), {q: ("mid", -11)})
        add("(c) seg %d: mid-point below 1.0, centre above" % q, _binade_mid(x, q, True), {q: ("mid", None)})
        add("(c) seg %d: mid-point at or above 1.0, centre below" % q, _binade_mid(x, q, False), {q: ("mid", None)})
    # (d) the last wave: 286 terms in the second half, the zero pad behind them
    w = _start_miss(x, 3, 40); w.update(_tail_terms())
    add("(d) last wave: start +40, mid hit, terms at 2048..2077", w, {3: ("mid", 0)})
    w = _start_miss(x, 3, -40); w.update(_mid_terms(x, 3, 33)); w.update(_tail_terms())
    add("(d) last wave: start -40, serial second half, terms at 2048..2077", w, {3: ("serial", 33)})
    w = _start_miss(x, 3, 40); w.update(S._triple(x, 3 * SEG + HALF - 1)); w.update(_tail_terms())
    add("(d) last wave: (big, -big, small) at 1791, 1792, 1793 and the tail", w, {3: None})
    w = _start_miss(x, 3, 40); w.update(_mid_terms(x, 3, -32)); w.update(S._triple(x, 3 * SEG + HALF + 2)); w.update(_tail_terms())
    add("(d) last wave: serial second half with the triple at 1794..1796 and the tail", w, {3: ("serial", -32)})
    # (e) two (three) missed segments in one mixer on one bit, resolved differently
    w = _start_miss(x, 1, 40); w.update(_mid_terms(x, 2, 33))
    add("(e) seg 1 mid hit, seg 2 serial half, seg 3 mid hit", w, {1: ("mid", 0), 2: ("serial", 33), 3: ("mid", 0)})
    w = _start_miss(x, 1, -40); w.update(_mid_terms(x, 1, -33)); w.update(_mid_terms(x, 3, 31))
    add("(e) seg 1 serial half, seg 2 mid hit, seg 3 mid hit at +31", w, {1: ("serial", -33), 2: ("mid", 0), 3: ("mid", 31)})
    mixers = [m for m in range(N_MIX0) if m != S.AUX_MIXER]
    for c, case in enumerate(cases):
        case.bit, case.mixer = c, mixers[c % len(mixers)]
    assert len(cases) == N_CRAFTED
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def crafted():
    """The crafted stream (one case per bit): the oracle's p and mixer outputs with the injection, the model's records. Read-only."""
    cases = crafted_cases()
    T = len(cases)
    probs = np.full((T, N_IN0), S.CRAFT_P, np.float32)
    sel = np.repeat(np.arange(T, dtype=np.uint64)[:, None], N_MIX, axis=1)
    bits = (np.arange(T) % 2).astype(np.uint8)
    inject = [(c.mixer, c.bit, i, v) for c in cases for i, v in sorted(c.weights.items())]
    p, mix, recs, rr = run(probs, sel, bits, inject)
    for a in (probs, sel, bits, p, mix, recs, rr):
        a.setflags(write=False)
    return {"cases": cases, "probs": probs, "sel": sel, "bits": bits, "p": p, "mix": mix, "recs": recs, "rr": rr}
