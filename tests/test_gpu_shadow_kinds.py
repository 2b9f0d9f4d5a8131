"""GPU: the pipeline's four kinds of shadow stages side by side on one handle (cmix_amd/csrc/pipeline_shadow.h). They are driven by
one implementation and a per-kind table, so what this pins is one kind's bookkeeping leaking into another's: each kind's own instance count, its own
unit of counting (the LSTM's vote counts bytes, the others bits), its own streams in the queue count when only some kinds are set back and set again
-- and a p that is the p of a handle without shadows, bit for bit."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

N_CHUNK, CHUNKS = 256, 3


def _run(shadows):
    """three chunks through a Pipeline with the fxcm stage on the device; shadows(pipe) sets them before the first chunk. -> (p, the four reports)"""
    import torch
    from cmix_amd import engine as E
    from cmix_amd import synth as S
    data = np.frombuffer(S.enwik_like(CHUNKS * N_CHUNK, 21), np.uint8)
    rng = np.random.default_rng(8)
    cols = (rng.integers(1, 4095, (8 * CHUNKS * N_CHUNK, 2078)).astype(np.float32) * np.float32(1.0 / 4095)).astype(np.float32)
    layer0 = torch.from_numpy(cols).cuda()
    p = torch.full((8 * CHUNKS * N_CHUNK,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pipe = E.Pipeline(np.ones(256, np.uint8), 0, max_chunk_bytes=N_CHUNK)
    try:
        pipe.enable_fxcm(None)
        shadows(pipe)
        for i in range(CHUNKS):
            a, b = i * N_CHUNK, (i + 1) * N_CHUNK
            pipe.submit(data[a:b].tobytes(), layer0[8 * a:8 * b], p[8 * a:8 * b])
        pipe.sync()
        reports = [pipe.shadow_report(), pipe.ctx_shadow_report(), pipe.lstm_shadow_report(), pipe.fxcm_shadow_report()]
        return p.cpu().numpy().copy(), reports
    finally:
        pipe.close()


def test_four_kinds_with_different_k_keep_their_own_books():
    from cmix_amd import engine as E
    q_start = E.hw_queues()
    p_plain, reports = _run(lambda pipe: None)
    assert [r["raw"] for r in reports] == [[0] * 8] * 4
    assert E.hw_queues() == q_start

    def shadows(pipe):
        q = E.hw_queues()
        pipe.set_fxcm_shadow(1)
        pipe.set_shadow(1)
        pipe.set_ctx_shadow(1)
        pipe.set_lstm_shadow(1)
        assert E.hw_queues() == q + 4
        pipe.set_ctx_shadow(0)
        pipe.set_shadow(0)
        assert E.hw_queues() == q + 2
        pipe.set_ctx_shadow(2)
        pipe.set_shadow(2)
        assert E.hw_queues() == q + 6

    p, (mix, ctx, lstm, fxcm) = _run(shadows)
    bits = 8 * CHUNKS * N_CHUNK
    assert mix["raw"] == [CHUNKS, bits, 3, 0, 0, 0, 0, 0]
    assert ctx["raw"] == [CHUNKS, bits, 3, 0, 0, 0, 0, 0]
    assert lstm["raw"] == [CHUNKS, CHUNKS * N_CHUNK, 2, 0, 0, 0, 0, 0]   # the LSTM's vote counts bytes
    assert fxcm["raw"] == [CHUNKS, bits, 2, 0, 0, 0, 0, 0]
    assert bits_equal(p, p_plain).all()
    assert E.hw_queues() == q_start
