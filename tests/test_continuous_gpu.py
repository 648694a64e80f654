"""The continuous call's kernels through the C ABI (cv2_wave_gate_chunk, cv2_wave_emit_chunk; cv2amd.join.WaveStream) against the numpy
restatement of the definitions (tests/_join_stream.py), bit for bit, under chunkings that must not matter.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

import _join_stream as RS

pytestmark = pytest.mark.gpu


def _noise(rng, n, amp):
    return (rng.standard_normal(n) * amp).astype(np.float32)


def _signals():
    """name -> three segments of 1000 .. 5000 samples"""
    rng = np.random.default_rng(11)
    out = {}
    # a quiet run of 3 frames between loud frames (held, then released); the segment ends 60 samples after its last loud frame
    a = _noise(rng, 240 * 12 + 60, 1e-5)
    a[0:1200] = _noise(rng, 1200, 0.3)
    a[1920:240 * 12] = _noise(rng, 240 * 12 - 1920, 0.2)
    b = _noise(rng, 4999, 1e-5)
    b[1300:2100] = _noise(rng, 800, 0.25)
    c = _noise(rng, 1000, 1e-5)
    c[333:700] = _noise(rng, 367, 0.4)
    out['held_and_released'] = [a, b, c]
    # an all-zero middle segment: no loud frame, kept whole
    out['zero_middle'] = [b.copy(), np.zeros(1500, np.float32), a.copy()]
    # NaN samples: one in a loud frame, one in a quiet one, one as a segment's first sample
    d, e = b.copy(), a.copy()
    d[1500], d[4000], e[0] = np.nan, np.nan, np.nan
    out['nan'] = [c.copy(), d, e]
    # a middle segment quieter than the gate's threshold against what came before, and a last one with a soft start
    f = _noise(rng, 2000, 1e-6)
    f[500:900] = _noise(rng, 400, 1e-4)
    h = _noise(rng, 3001, 1e-6)
    h[1500:1800] = _noise(rng, 300, 5e-3)
    h[2000:2600] = _noise(rng, 600, 0.5)
    out['quiet_middle'] = [a.copy(), f, h]
    return out


SIGNALS = _signals()


def _cuts(segs, mode, rng):
    if mode == 'whole':
        return [[] for _ in segs]
    if mode == 'one_sample':                                                  # 1-sample chunks for the shortest segment
        j = int(np.argmin([len(s) for s in segs]))
        return [list(range(1, len(s))) if i == j else [len(s) // 2] for i, s in enumerate(segs)]
    if mode == 'frame_edges':
        return [sorted({239, 240, 241, 479, 480, 481, 240 * 7 - 1, 240 * 7, 240 * 7 + 1, len(s) - 1}) for s in segs]
    return [sorted(set(rng.integers(1, len(s), size=int(rng.integers(2, 9))).tolist())) for s in segs]


def _run(segs, join, cuts, dev):
    """-> (the stream as one numpy array, spans): every chunk written into ONE buffer behind the previous one, so that an odd pause puts
    the later destinations off 16-byte alignment; after every chunk the device's held count is the planner's"""
    from cv2amd.join import WaveStream
    ws = WaveStream(join, len(segs), dev)
    pause = ws.plan.pause
    buf = torch.full((sum(len(s) for s in segs) + pause * len(segs) + 8,), 7.0, dtype=torch.float32, device=dev)
    pos = 0
    for i, s in enumerate(segs):
        t = torch.from_numpy(s).to(dev)
        edges = [0] + [c for c in cuts[i] if 0 < c < len(s)] + [len(s)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            n_before = ws.launches
            end = hi == len(s)
            o = ws.chunk(t[lo:hi], end, into=(buf, pos))
            pos += o.numel()
            assert ws.launches > n_before
            st = ws.state.cpu().tolist()
            held = 0 if end else ws.plan.n_held                               # (a segment's end leaves nothing held)
            assert st[5] <= held and st[5] == held and (end or st[6] == ws.plan.e), (i, hi, st)
    assert ws.plan.done and float(buf[pos]) == 7.0                            # nothing was written behind the stream
    spans = list(ws.plan.spans)
    ws.close()
    return buf[:pos].cpu().numpy(), spans


@pytest.mark.parametrize('name', sorted(SIGNALS))
@pytest.mark.parametrize('settings', [dict(pause_ms=0, trim_db=40, fade_ms=5), dict(pause_ms=7 / 24, trim_db=40, fade_ms=0),
                                      dict(pause_ms=301 / 24, trim_db=26.5), dict(pause_ms=5 / 24)])
def test_stream_equals_the_restatement_whatever_the_chunks(name, settings):
    from cv2amd.join import Join
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', torch.cuda.current_device())
    segs, join = SIGNALS[name], Join(**settings)
    pause, F, g = join.resolve()
    assert F == (0 if settings.get('trim_db') is None else (120 if settings.get('fade_ms') != 0 else 0)) and pause in (0, 7, 301, 5)
    want, spans = RS.stream(segs, None if g is None else np.float32(g), pause, F)
    if g is not None:
        assert want.size < sum(len(s) for s in segs) + 2 * pause              # the gate did cut something
    rng = np.random.default_rng(5)
    for mode in ('whole', 'one_sample', 'frame_edges', 'random', 'random'):
        got, got_spans = _run(segs, join, _cuts(segs, mode, rng), dev)
        assert got_spans == spans, mode
        assert got.size == want.size and np.array_equal(got.view(np.int32), want.view(np.int32)), (mode, int(np.argmax(got.view(np.int32) != want.view(np.int32)[:got.size])) if got.size == want.size else (got.size, want.size))


def test_a_plain_chunk_is_handed_on_untouched_and_the_entry_points_refuse_bad_ranges():
    import ctypes as C
    from cv2amd import lib as L
    from cv2amd import join as J
    dev = torch.device('cuda', torch.cuda.current_device())
    ws = J.WaveStream(J.Join(pause_ms=1), 2, dev)
    x = torch.randn(1, 1000, device=dev)
    o = ws.chunk(x, False)
    assert o.data_ptr() == x.data_ptr() and ws.launches == 0                  # no gate, nothing held, no pause yet: no launch
    o = ws.chunk(x, True)
    assert ws.launches == 1 and o.numel() == 1024 and torch.equal(o[:1000], x[0]) and int(o[1000:].view(torch.int32).abs().sum()) == 0
    lib = L.lib()
    st, rec, buf = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4096, device=dev)
    p, sp = buf.data_ptr(), L.stream_ptr()
    assert lib.cv2_wave_gate_chunk(st.data_ptr(), None, 0, 0, p, 1000, 0, 6, 1, 0.01, rec.data_ptr(), sp) == -1        # frame 5 has no sample yet
    assert lib.cv2_wave_gate_chunk(st.data_ptr(), None, 480, 0, p, 1000, 1, 2, 0, 0.01, rec.data_ptr(), sp) == -1      # frame 1 starts before the held samples
    assert lib.cv2_wave_gate_chunk(st.data_ptr(), None, 0, 0, p, 1000, 0, 4, 1, 1.5, rec.data_ptr(), sp) == -1
    dst, held = torch.zeros(2048, device=dev), torch.zeros(2048, device=dev)

    def emit(**kw):
        a = J.WaveEmit(None, p, None, dst.data_ptr(), held.data_ptr(), 0, 0, 1000, 0, 500, -1, -1, 0, 0, 500, 2048, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.cv2_wave_emit_chunk(st.data_ptr(), C.byref(a), sp)
    assert emit() == 0
    for bad in (dict(e1=1001), dict(keep_from=400), dict(held_cap=499), dict(F=121), dict(F=120, fade_out_end=400), dict(n_zero=-1),
                dict(held_dst=p + 400), dict(dst=p), dict(F=120, fade_out_end=500, e0=400)):
        assert emit(**bad) == -1, bad
    torch.cuda.synchronize()
    assert st.cpu().tolist()[5:7] == [500, 500]
