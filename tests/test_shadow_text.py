"""CPU: the words of the pipeline's four kinds of shadow stages (cmix_amd/csrc/cmx_shadow_text.h), built for the host (tests/host/shadow_text.cpp) and
compared with the literal texts that the four separate copies of this code produced before they became one table: a vote's record in words at every
edge of each kind's column naming, a timed-out hand-off as cmx_pipeline_wait and cmx_pipeline_sync say it, "no such instance", the queue budget, and
the repair log's entries. Also without a device: every shadow entry point of the library on a null handle, and the shadow methods of Pipeline and
Predictor with their signatures, against lists recorded from the same code."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "shadow_text.cpp")
NONE = (1 << 64) - 1   # a vote without a majority
MIX, CTX, LSTM, FXCM = range(4)

VOTE = [   # (kind, position, column, odd, text) of the record [5, 4096, 3, 1, position, column, odd, 7]
    (0, 1234, 0, NONE, "shadow vote: the 3 mixing-network instances disagree in 7 value(s) of the chunk, first at stream bit 1234, mixer 0: no majority between 3 instances (the stream's output is void)"),
    (0, 1234, 0, 0, "shadow vote: the 3 mixing-network instances disagree in 7 value(s) of the chunk, first at stream bit 1234, mixer 0: instance 0 is the odd one (the stream's own network) (the stream's output is void)"),
    (0, 1234, 0, 1, "shadow vote: the 3 mixing-network instances disagree in 7 value(s) of the chunk, first at stream bit 1234, mixer 0: instance 1 is the odd one (the stream's output is void)"),
    (0, 1234, 46, 1, "shadow vote: the 3 mixing-network instances disagree in 7 value(s) of the chunk, first at stream bit 1234, mixer 46: instance 1 is the odd one (the stream's output is void)"),
    (0, 1234, 47, 1, "shadow vote: the 3 mixing-network instances disagree in 7 value(s) of the chunk, first at stream bit 1234, final p: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 0, NONE, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 0: no majority between 3 instances (the stream's output is void)"),
    (1, 1234, 0, 0, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 0: instance 0 is the odd one (the stream's own stage) (the stream's output is void)"),
    (1, 1234, 0, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 0: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 2, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 2: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 3, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 2025: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 53, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, layer-0 column 2075: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 54, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, selector 0: instance 1 is the odd one (the stream's output is void)"),
    (1, 1234, 100, 1, "context shadow vote: the 3 context-stage instances disagree in 7 value(s) of the chunk, first at stream bit 1234, selector 46: instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 0, NONE, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, distribution entry 0: no majority between 3 instances (the stream's output is void)"),
    (2, 1234, 0, 0, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, distribution entry 0: instance 0 is the odd one (the stream's own stage) (the stream's output is void)"),
    (2, 1234, 0, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, distribution entry 0: instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 255, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, distribution entry 255: instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 256, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, bit 0's prediction (layer-0 column 2077): instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 263, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, bit 7's prediction (layer-0 column 2077): instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 264, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, bit 0's ex: instance 1 is the odd one (the stream's output is void)"),
    (2, 1234, 271, 1, "LSTM shadow vote: the 3 LSTM-stage instances disagree in 7 value(s) of the chunk, first at stream byte 1234, bit 7's ex: instance 1 is the odd one (the stream's output is void)"),
    (3, 301, 0, NONE, "fxcm shadow vote: the 3 fxcm-stage instances disagree in 7 value(s) of the chunk, first at stream bit 301 (byte 37, bit 5), fxcm column 0 (layer-0 column 3): no majority between 3 instances (the stream's output is void)"),
    (3, 301, 0, 0, "fxcm shadow vote: the 3 fxcm-stage instances disagree in 7 value(s) of the chunk, first at stream bit 301 (byte 37, bit 5), fxcm column 0 (layer-0 column 3): instance 0 is the odd one (the stream's own stage) (the stream's output is void)"),
    (3, 301, 0, 1, "fxcm shadow vote: the 3 fxcm-stage instances disagree in 7 value(s) of the chunk, first at stream bit 301 (byte 37, bit 5), fxcm column 0 (layer-0 column 3): instance 1 is the odd one (the stream's output is void)"),
    (3, 301, 430, 1, "fxcm shadow vote: the 3 fxcm-stage instances disagree in 7 value(s) of the chunk, first at stream bit 301 (byte 37, bit 5), fxcm column 430 (layer-0 column 433): instance 1 is the odd one (the stream's output is void)"),
]
TIMEOUT = [   # (kind, instance, chunk or -1 for cmx_pipeline_sync's form, text)
    (0, 1, 41, "cmx_pipeline_wait: an in-launch hand-off of shadow mixing network 1 timed out (workgroups not co-resident?): the vote is void from chunk 41 on"),
    (2, 1, 41, "cmx_pipeline_wait: an in-launch hand-off of the LSTM kernels of shadow instance 1 timed out (workgroups not co-resident?): the LSTM vote is void from chunk 41 on"),
    (2, 1, -1, "cmx_pipeline_sync: an in-launch hand-off of the LSTM kernels of shadow instance 1 timed out (workgroups not co-resident?): the LSTM vote is void"),
    (3, 1, 41, "cmx_pipeline_wait: an in-launch hand-off of the fxcm kernel of shadow instance 1 timed out (workgroups not co-resident?): the fxcm vote is void from chunk 41 on"),
    (3, 1, -1, "cmx_pipeline_sync: an in-launch hand-off of the fxcm kernel of shadow instance 1 timed out (workgroups not co-resident?): the fxcm vote is void"),
    (0, 2, 41, "cmx_pipeline_wait: an in-launch hand-off of shadow mixing network 2 timed out (workgroups not co-resident?): the vote is void from chunk 41 on"),
    (2, 2, 41, "cmx_pipeline_wait: an in-launch hand-off of the LSTM kernels of shadow instance 2 timed out (workgroups not co-resident?): the LSTM vote is void from chunk 41 on"),
    (2, 2, -1, "cmx_pipeline_sync: an in-launch hand-off of the LSTM kernels of shadow instance 2 timed out (workgroups not co-resident?): the LSTM vote is void"),
    (3, 2, 41, "cmx_pipeline_wait: an in-launch hand-off of the fxcm kernel of shadow instance 2 timed out (workgroups not co-resident?): the fxcm vote is void from chunk 41 on"),
    (3, 2, -1, "cmx_pipeline_sync: an in-launch hand-off of the fxcm kernel of shadow instance 2 timed out (workgroups not co-resident?): the fxcm vote is void"),
]
NO_INSTANCE = [   # (kind, text)
    (0, "cmx_pipeline_shadow_state_diff: no such instance (0 = the stream's network, 1.. = the shadows, which exist from the first chunk on)"),
    (1, "cmx_pipeline_ctx_shadow_state_diff: no such instance (0 = the stream's own stage, 1.. = the shadows, which exist from the first chunk on)"),
    (2, "cmx_pipeline_lstm_shadow_state_diff: no such instance (0 = the stream's own stage, 1.. = the shadows, which exist from the first chunk on)"),
    (3, "cmx_pipeline_fxcm_shadow_state_diff: no such instance (0 = the stream's own stage, 1.. = the shadows, which exist from the first chunk or pretrain on)"),
]
QUEUES = [   # (kind, text) for 31 queues held on device 2, k = 2, the limit 32
    (0, "cmx_pipeline_set_shadow: this process holds 31 dedicated hardware queues on device 2 and 2 shadow mixing network(s) need one each, the limit is 32"),
    (1, "cmx_pipeline_set_ctx_shadow: this process holds 31 dedicated hardware queues on device 2 and 2 shadow context stage(s) need one each, the limit is 32"),
    (2, "cmx_pipeline_set_lstm_shadow: this process holds 31 dedicated hardware queues on device 2 and 2 shadow LSTM stage(s) need one each, the limit is 32"),
    (3, "cmx_pipeline_set_fxcm_shadow: this process holds 31 dedicated hardware queues on device 2 and 2 shadow fxcm stage(s) need one each, the limit is 32"),
]
REPAIR = [   # (layer-0 mask, layers-1/2 mask, origin text, entry text) of the entry [9, 73000, column 46 / 47 / 46, 2, 1, 12, ..., masks at 12 and 13]
    (0x100020, 0x0, "mixer 5", "chunk 9, stream bit 73000, mixer 46, instance 2 odd, 12 state word(s) repaired, origin mixer 5"),
    (0x0, 0x100008, "mixer 29", "chunk 9, stream bit 73000, final p, instance 2 odd, 12 state word(s) repaired, origin mixer 29"),
    (0x0, 0x0, "no mixer row (tables / scalars only)", "chunk 9, stream bit 73000, mixer 46, instance 2 odd, 12 state word(s) repaired, origin no mixer row (tables / scalars only)"),
]

NULL_HANDLE = [   # (entry point, its last_error() on a null handle)
    ("cmx_pipeline_set_shadow", "cmx_pipeline_set_shadow: null handle"),
    ("cmx_pipeline_shadow_report", "cmx_pipeline_shadow_report: bad argument"),
    ("cmx_pipeline_shadow_values", "cmx_pipeline_shadow_values: bad argument"),
    ("cmx_pipeline_shadow_state_diff", "cmx_pipeline_shadow_state_diff: bad argument"),
    ("cmx_pipeline_debug_shadow_xor", "cmx_pipeline_debug_shadow_xor: null handle"),
    ("cmx_set_shadow", "cmx_set_shadow: null handle"),
    ("cmx_shadow_report", "cmx_shadow_report: bad argument"),
    ("cmx_pipeline_set_ctx_shadow", "cmx_pipeline_set_ctx_shadow: null handle"),
    ("cmx_pipeline_ctx_shadow_report", "cmx_pipeline_ctx_shadow_report: bad argument"),
    ("cmx_pipeline_ctx_shadow_values", "cmx_pipeline_ctx_shadow_values: bad argument"),
    ("cmx_pipeline_ctx_shadow_state_diff", "cmx_pipeline_ctx_shadow_state_diff: bad argument"),
    ("cmx_pipeline_debug_ctx_shadow_xor", "cmx_pipeline_debug_ctx_shadow_xor: null handle"),
    ("cmx_set_ctx_shadow", "cmx_set_ctx_shadow: null handle"),
    ("cmx_ctx_shadow_report", "cmx_ctx_shadow_report: bad argument"),
    ("cmx_pipeline_set_lstm_shadow", "cmx_pipeline_set_lstm_shadow: null handle"),
    ("cmx_pipeline_lstm_shadow_report", "cmx_pipeline_lstm_shadow_report: bad argument"),
    ("cmx_pipeline_lstm_shadow_values", "cmx_pipeline_lstm_shadow_values: bad argument"),
    ("cmx_pipeline_lstm_shadow_state_diff", "cmx_pipeline_lstm_shadow_state_diff: bad argument"),
    ("cmx_pipeline_debug_lstm_shadow_xor", "cmx_pipeline_debug_lstm_shadow_xor: null handle"),
    ("cmx_set_lstm_shadow", "cmx_set_lstm_shadow: null handle"),
    ("cmx_lstm_shadow_report", "cmx_lstm_shadow_report: bad argument"),
    ("cmx_pipeline_set_fxcm_shadow", "cmx_pipeline_set_fxcm_shadow: null handle"),
    ("cmx_pipeline_fxcm_shadow_report", "cmx_pipeline_fxcm_shadow_report: bad argument"),
    ("cmx_pipeline_fxcm_shadow_values", "cmx_pipeline_fxcm_shadow_values: bad argument"),
    ("cmx_pipeline_fxcm_shadow_state_diff", "cmx_pipeline_fxcm_shadow_state_diff: bad argument"),
    ("cmx_pipeline_debug_fxcm_shadow_xor", "cmx_pipeline_debug_fxcm_shadow_xor: null handle"),
    ("cmx_set_fxcm_shadow", "cmx_set_fxcm_shadow: null handle"),
    ("cmx_fxcm_shadow_report", "cmx_fxcm_shadow_report: bad argument"),
    ("cmx_debug_shadow_xor", "cmx_debug_shadow_xor: null handle"),
    ("cmx_debug_ctx_shadow_xor", "cmx_debug_ctx_shadow_xor: null handle"),
]
PIPELINE_METHODS = {   # name: str(inspect.signature)
    "ctx_shadow_report": "(self)",
    "ctx_shadow_state_diff": "(self, a, b)",
    "ctx_shadow_values": "(self)",
    "debug_ctx_shadow_xor": "(self, instance, region, lane, index, xor_mask)",
    "debug_fxcm_shadow_xor": "(self, instance, region, index, xor_mask)",
    "debug_lstm_shadow_xor": "(self, instance, region, index, xor_mask)",
    "debug_shadow_xor": "(self, instance, region, mixer, row, index, xor_mask)",
    "fxcm_shadow_report": "(self)",
    "fxcm_shadow_state_diff": "(self, a, b)",
    "fxcm_shadow_values": "(self)",
    "lstm_shadow_report": "(self)",
    "lstm_shadow_state_diff": "(self, a, b)",
    "lstm_shadow_values": "(self)",
    "set_ctx_shadow": "(self, k)",
    "set_fxcm_shadow": "(self, k)",
    "set_lstm_shadow": "(self, k)",
    "set_shadow": "(self, k)",
    "set_shadow_repair": "(self, max_repairs)",
    "shadow_repairs": "(self)",
    "shadow_report": "(self)",
    "shadow_state_diff": "(self, a, b)",
    "shadow_values": "(self)",
}
PREDICTOR_METHODS = {   # name: str(inspect.signature)
    "ctx_shadow_report": "(self)",
    "debug_ctx_shadow_xor": "(self, after_chunk, instance, region, lane, index, xor_mask)",
    "debug_shadow_xor": "(self, after_chunk, instance, region, mixer, row, index, xor_mask)",
    "fxcm_shadow_report": "(self)",
    "lstm_shadow_report": "(self)",
    "set_ctx_shadow": "(self, k)",
    "set_fxcm_shadow": "(self, k)",
    "set_lstm_shadow": "(self, k)",
    "set_shadow": "(self, k)",
    "set_shadow_repair": "(self, max_repairs)",
    "shadow_repairs": "(self)",
    "shadow_report": "(self)",
}


@pytest.fixture(scope="module")
def st(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shadow_text") / "libshadowtext.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    for name, args in (("st_vote", [C.c_int, C.c_void_p]), ("st_timeout", [C.c_int, C.c_int, C.c_longlong]), ("st_no_instance", [C.c_int, C.c_char_p, C.c_char_p]),
                       ("st_queue", [C.c_int] * 5), ("st_origin", [C.c_uint64, C.c_uint64]), ("st_repair_entry", [C.c_void_p])):
        getattr(L, name).restype = C.c_char_p
        getattr(L, name).argtypes = args
    return L


def test_the_cases_cover_what_they_should():
    """the edges of every kind's column naming, all three outcomes per kind, both shadow instances in both forms"""
    cols = {k: sorted({c for kk, _, c, _, _ in VOTE if kk == k}) for k in range(4)}
    assert cols == {MIX: [0, 46, 47], CTX: [0, 2, 3, 53, 54, 100], LSTM: [0, 255, 256, 263, 264, 271], FXCM: [0, 430]}
    assert all({odd for kk, _, _, odd, _ in VOTE if kk == k} == {NONE, 0, 1} for k in range(4))
    assert all(pos % 8 == 5 for kk, pos, _, _, _ in VOTE if kk == FXCM)   # both the byte and the bit show
    assert {(k, i, c < 0) for k, i, c, _ in TIMEOUT} == {(MIX, 1, False), (MIX, 2, False)} | {(k, i, s) for k in (LSTM, FXCM) for i in (1, 2) for s in (False, True)}


@pytest.mark.parametrize("kind, pos, col, odd, text", VOTE)
def test_vote_text(st, kind, pos, col, odd, text):
    r = (C.c_uint64 * 8)(5, 4096, 3, 1, pos, col, odd, 7)
    assert st.st_vote(kind, r).decode() == text


@pytest.mark.parametrize("kind, instance, chunk, text", TIMEOUT)
def test_timed_out_hand_off_text(st, kind, instance, chunk, text):
    assert st.st_timeout(kind, instance, chunk).decode() == text


def test_no_such_instance_and_queue_budget_text(st):
    for kind, text in NO_INSTANCE:
        assert st.st_no_instance(kind, b"cmx_pipeline_", b"_state_diff").decode() == text
        xor = text.replace("cmx_pipeline_", "cmx_pipeline_debug_", 1).replace("_state_diff:", "_xor:", 1)   # the same words behind the other function's name
        assert st.st_no_instance(kind, b"cmx_pipeline_debug_", b"_xor").decode() == xor
    for kind, text in QUEUES:
        assert st.st_queue(kind, 31, 2, 2, 32).decode() == text


def test_repair_entry_and_origin_text(st):
    for (m0, m12, origin, entry), col in zip(REPAIR, (46, 47, 46)):
        assert st.st_origin(m0, m12).decode() == origin
        e = (C.c_uint64 * 16)(9, 73000, col, 2, 1, 12, 0, 0, 0, 0, 0, 0, m0, m12, 1, 0)
        assert st.st_repair_entry(e).decode() == entry


def test_every_shadow_entry_point_refuses_a_null_handle():
    from cmix_amd import engine as E
    L = E.lib()
    out, words = (C.c_uint64 * 20)(), (C.c_uint32 * (3 * 431))()
    values = {"shadow": (words, None, None), "ctx_shadow": (words, None), "lstm_shadow": (words, None), "fxcm_shadow": (words, None, None)}
    xor = {"shadow": (0, 0, 0), "ctx_shadow": (0, 0), "lstm_shadow": (0,), "fxcm_shadow": (0,)}
    args = {}
    for stem in values:
        args.update({"cmx_pipeline_set_" + stem: (1,), "cmx_pipeline_" + stem + "_report": (out,), "cmx_pipeline_" + stem + "_values": values[stem],
                     "cmx_pipeline_" + stem + "_state_diff": (0, 1, out), "cmx_pipeline_debug_" + stem + "_xor": (0, 0) + xor[stem] + (1,),
                     "cmx_set_" + stem: (1,), "cmx_" + stem + "_report": (out,)})
    args.update({"cmx_debug_shadow_xor": (0, 0, 0, 0, 0, 0, 1), "cmx_debug_ctx_shadow_xor": (0, 0, 0, 0, 0, 1)})
    assert sorted(args) == sorted(name for name, _ in NULL_HANDLE) and len(args) == 30
    for name, text in NULL_HANDLE:
        assert getattr(L, name)(None, *args[name]) == 1, name
        assert E.last_error() == text


def test_pipeline_and_predictor_keep_their_shadow_methods():
    from cmix_amd import engine as E
    for cls, want in ((E.Pipeline, PIPELINE_METHODS), (E.Predictor, PREDICTOR_METHODS)):
        have = {m: str(inspect.signature(getattr(cls, m))) for m in dir(cls) if "shadow" in m and not m.startswith("_")}
        assert have == want
        assert all(getattr(cls, m).__doc__ for m in want)
