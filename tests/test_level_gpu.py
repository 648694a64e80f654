"""k_level (cv2_level_chunk / cv2_level_chunk_batch) and k_level_peak (cv2_level_peak_batch) on the device: chunk invariance bit for bit,
the values against the numpy restatement of the definition (tests/_level.py) -- bit-equal where the restatement's sum is zero, within a
derived bound elsewhere --, the ceiling, the special values, the peak target, the batched form against single calls, refused arguments.
Run with -m gpu."""
import numpy as np
import pytest
import torch

import _level as R

pytestmark = pytest.mark.gpu

GUARD = 9
C6 = R.db(-6.0)                      # the ceiling most cases run under


def _guarded(x, off):
    """x inside a larger device buffer whose base is 16-byte aligned, `off` elements in, NaN around it -> (buffer, view)"""
    buf = torch.full((off + x.numel() + GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    buf[off:off + x.numel()] = x
    return buf, buf[off:off + x.numel()]


class _Call:
    """What the scheduler keeps per call: the planner's state and the retained samples -- here with the source, the tail and every
    destination at changing 4-byte offsets mod 16 inside guarded buffers."""

    def __init__(self, sig, L, Ge=1.0, c=C6, rot=0, peak=None, T=None, seen=None):
        from cv2amd import level as LV
        self.LV, self.Ge, self.c, self.rot, self.peak, self.T = LV, float(Ge), float(c), rot, peak, T
        self.src_off = rot % 4
        self.src_buf, self.src = _guarded(sig, self.src_off)
        self.st, self.tail, self.pos, self.k = LV.LevelState(L), None, 0, 0
        self.w = LV.weight_table('cuda', L)
        self.seen = seen if seen is not None else set()

    def job(self, n_new, final):
        """-> (record, destination buffer, plan) of the next chunk; nothing advances"""
        fresh = self.src[self.pos:self.pos + n_new]
        n0, n_emit, first_needed = self.LV.plan(self.st, n_new, final)
        off = (self.rot + self.k) % 4 + 4 * ((self.k // 4) % 2)
        buf, dst = _guarded(torch.zeros(n_emit, device='cuda'), off)
        dst.fill_(float('nan'))
        a = self.LV.level_args(self.st, self.Ge, self.c, self.tail, fresh, dst, n0, n_emit, final, self.w, self.peak, self.T)
        if n_emit:
            self.seen.add(('dst', a.dst % 16))
        if n_new:
            self.seen.add(('src', a.fresh % 16))
        if a.n_tail:
            self.seen.add(('tail', a.tail % 16))
        return a, (buf, off, n_emit), (n_new, n_emit, first_needed, final, fresh)

    def advance(self, plan):
        n_new, n_emit, first_needed, final, fresh = plan
        both = fresh if self.tail is None else torch.cat([self.tail, fresh])
        keep = both[first_needed - self.st.first:]
        assert keep.numel() <= 2 * self.st.L
        self.tail = _guarded(keep, (self.rot + self.k + 1) % 4)[1] if keep.numel() else None
        self.st.commit(n_new, n_emit, first_needed, final)
        self.pos += n_new
        self.k += 1

    def emitted(self, dst):
        buf, off, n_emit = dst
        assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + n_emit:]).all(), 'wrote outside [dst, dst + n_emit)'
        return buf[off:off + n_emit].clone()

    def guards_intact(self):
        o = self.src_off
        return bool(torch.isnan(self.src_buf[:o]).all() and torch.isnan(self.src_buf[o + self.src.numel():]).all())


def _run(sig, L, chunks, **kw):
    c, outs = _Call(sig, L, **kw), []
    for k, n_new in enumerate(chunks):
        a, dst, plan = c.job(n_new, k == len(chunks) - 1)
        c.LV.level_chunks([a])
        outs.append(c.emitted(dst))
        c.advance(plan)
    assert c.guards_intact()
    return torch.cat(outs)


def _dev(s):
    return torch.from_numpy(np.ascontiguousarray(s)).cuda()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _check_values(y, s, Ge, c, L, tag):
    """the device's y against the restatement.
    Where the restatement's acc is 0 (no sample within the look-ahead is over): g = min(1, r) = 1 there (r < 1 only at an over, whose own
    d > 0 makes acc > 0 through w[j] > 0), so y = fl(1 * x) = x, bit for bit.
    Elsewhere: the device sums acc as one chain of L + 1 fmaf.  Every partial sum is <= sum_j w[j] D <= (1 + 2^-24 (L + 1)) (D <= 1, the
    float32 weights sum to 1 within their own roundings), and each fmaf rounds its partial sum once, by <= 2^-24 of it: |acc - acc64| <=
    (L + 1) 2^-24 (1 + ...), the float64 sum being exact at this scale.  1 - acc is one more rounding of a value <= 1: |g - g64| <=
    (L + 2) 2^-24 (1 + ...) <= (L + 3) 2^-24 (r is the same float on both sides, and max / min are 1-Lipschitz).  y = fl(g x) rounds once
    more, by <= 2^-24 |g x| <= 2^-24 |x|: |y - y64| <= (L + 4) 2^-24 |x| before the clamp, which is 1-Lipschitz; 2^-24 c covers the
    clamp's own constant seen as a float64."""
    ref = R.level64(s, Ge, c, L)
    x, y64 = ref['x'], ref['y']
    zero = ref['acc'] == 0.0
    fin = np.isfinite(x)
    assert np.array_equal(_bits(y[zero & fin]), _bits(x[zero & fin])), f'{tag}: not the input where nothing is over within the look-ahead'
    assert np.array_equal(zero & fin, R.quiet(s, Ge, c, L) & fin), f'{tag}: the restatement itself'
    err = np.abs(y[fin].astype(np.float64) - y64[fin])
    bound = (L + 4) * R.U * np.abs(x[fin].astype(np.float64)) + R.U * float(c)
    assert (err <= bound).all(), f'{tag}: worst error {float((err / bound).max()):.3f} of the bound'
    assert (np.abs(y) <= np.float32(c)).all(), f'{tag}: a sample above the ceiling'
    # the special values: NaN -> +0, +-Inf -> +-c
    nan, inf = np.isnan(x), np.isinf(x)
    assert np.array_equal(_bits(y[nan]), np.zeros(int(nan.sum()), dtype=np.uint32))
    assert np.array_equal(y[inf], np.copysign(np.float32(c), x[inf]))
    return ref


@pytest.mark.parametrize('L', R.LOOKAHEADS)
def test_chunk_invariance_and_values(L):
    seen = set()
    for rot, n in enumerate(R.lengths(L)):
        s = R.bursts(n)
        sig = _dev(s)
        once = _run(sig, L, [n], rot=rot, seen=seen)
        assert once.shape == (n,)
        for k, (name, chunks) in enumerate(R.chunkings(n, L).items()):
            got = _run(sig, L, chunks, rot=rot + k + 1, seen=seen)
            assert torch.equal(got.view(torch.int32), once.view(torch.int32)), f'L={L} N={n}: "{name}" differs from the one-shot result'
        y = once.cpu().numpy()
        _check_values(y, s, 1.0, C6, L, f'L={L} N={n}')
        if n > 2 * L + 1:
            assert float(np.abs(y).max()) == float(C6), 'the burst reaches the ceiling exactly'
    for what in ('dst', 'src', 'tail'):
        assert {al for w, al in seen if w == what} == {0, 4, 8, 12}, f'{what}: every 4-byte offset mod 16'


@pytest.mark.parametrize('L', R.LOOKAHEADS)
def test_other_signals(L):
    n = 2 * 1024 + L + 3
    cases = {'all zero': (np.zeros(n, dtype=np.float32), 1.0, C6), 'under the ceiling': (R.sine(n, 0.45), 1.0, C6),
             'specials': (R.specials(n), 1.0, C6), 'gain +6.5 dB': (R.bursts(n), R.db(6.5), R.db(-1.0)),
             'gain -7 dB': (R.bursts(n), R.db(-7.0), R.db(-12.0)), 'specials, short': (R.specials(L + 1), R.db(3.0), C6)}
    for k, (name, (s, Ge, c)) in enumerate(cases.items()):
        sig = _dev(s)
        once = _run(sig, L, [len(s)], Ge=Ge, c=c, rot=k)
        for cname in ('ragged', 'shorter than L'):
            got = _run(sig, L, R.chunkings(len(s), L)[cname], Ge=Ge, c=c, rot=k + 1)
            assert torch.equal(got.view(torch.int32), once.view(torch.int32)), f'L={L} {name}: "{cname}" differs from the one-shot result'
        y = once.cpu().numpy()
        _check_values(y, s, Ge, c, L, f'L={L} {name}')
        if name in ('all zero', 'under the ceiling'):
            assert np.array_equal(_bits(y), _bits(s)), f'{name}: a sample that needed no change came out as another float'


@pytest.mark.parametrize('L', R.LOOKAHEADS)
def test_gain_curve(L):
    """magnitudes that are powers of two under c = 0.5 with Ge = 1: r, d and g x are exact, so y / x IS the device's g (no clamp acts:
    |g x| <= r |x| = c exactly) -- held to |g - g64| <= (L + 3) 2^-24 (the derivation: _check_values)."""
    n = 2 * 1024 + L + 3
    s = R.pow2(n, seed=L)
    y = _run(_dev(s), L, R.ragged(n), c=0.5, rot=2).cpu().numpy()
    ref = _check_values(y, s, 1.0, 0.5, L, f'L={L} powers of two')
    g = y.astype(np.float64) / s.astype(np.float64)
    assert np.array_equal((g * s.astype(np.float64)).astype(np.float32), y)
    err = np.abs(g - ref['g'])
    print(f'L={L}: worst |g - g64| = {err.max() / R.U:.2f} x 2^-24, bound {L + 3}')
    assert (err <= (L + 3) * R.U).all() and (ref['acc'] > 0).sum() > n // 4
    over = np.abs(s) > 0.5                                                     # (D[n - j] >= d[n] for every j: the smoothed reduction is at least the sample's own)
    assert (np.abs(y[over]) <= 0.5).all() and (np.abs(y[over]) > 0.5 * 0.125).all()


def test_peak_target():
    """P bit-equal to numpy's maximum (NaN counting as 0), from guarded sources at every offset; the level kernel reads P from device
    memory: the result is the definition's under Ge = fl(G fl(T / P))."""
    from cv2amd import level as LV
    L, G, c, T = 120, R.db(-2.0), R.db(-1.0), R.db(-3.0)
    sigs = [R.specials(5000)[:4999] * np.float32(0.2), R.bursts(4097), R.sine(1, 0.3) + np.float32(0.01), np.zeros(777, dtype=np.float32), R.sine(4096, 0.07)]
    sigs[0] = np.where(np.isinf(sigs[0]), np.float32(0.9), sigs[0]).astype(np.float32)      # (NaN stays: it counts as 0)
    bufs = [_guarded(_dev(s), k % 4 + 1) for k, s in enumerate(sigs)]
    peaks = LV.level_peaks([v for _b, v in bufs])
    want = np.array([R.peak(s) for s in sigs], dtype=np.float32)
    assert np.array_equal(_bits(peaks.cpu().numpy()), _bits(want)) and want[3] == 0 and want[0] == np.float32(0.9)
    assert np.isnan(sigs[0]).any()
    for k, s in enumerate(sigs):
        b, v = bufs[k]
        assert torch.isnan(b[:k % 4 + 1]).all() and torch.isnan(b[k % 4 + 1 + len(s):]).all()
        y = _run(v.clone(), L, [len(s)], Ge=G, c=c, peak=peaks[k:k + 1], T=T, rot=k).cpu().numpy()
        Ge = R.gain(G, want[k], T)
        assert Ge == G if want[k] == 0 else Ge != G
        ref = _check_values(y, s, Ge, c, L, f'peak target, signal {k}')
        if want[k] > 0 and not np.isnan(s).any():
            # the call's peak sits at G T within three roundings (T / P, G Gp, Ge P), each <= 2^-24 relative; nothing is over the ceiling
            gt = float(G) * float(T)
            assert abs(float(np.abs(y).max()) - gt) <= 3.001 * R.U * gt and (ref['acc'] == 0).all()
            assert float(np.abs(y).max()) == float(np.float32(Ge * want[k]))


@pytest.mark.parametrize('n_calls', (1, 3, 8))
def test_batched_equals_single_calls(n_calls):
    """calls of different length, look-ahead, gain and ceiling, each after a first chunk, in ONE launch against the single launches"""
    from cv2amd import level as LV
    cases = [(4803, 120, 1.0, C6, 480, 2000, False), (1000, 24, R.db(4.0), R.db(-1.0), 300, 700, True), (257, 240, 1.0, R.db(-12.0), 100, 157, True),
             (4803, 240, R.db(-3.0), R.db(-3.0), 2500, 2303, True), (1000, 48, 1.0, 1.0, 1, 999, True), (256, 24, R.db(12.0), C6, 100, 150, False),
             (4803, 72, 1.0, R.db(-2.0), 4000, 803, True), (300, 120, 1.0, C6, 299, 1, True)][:n_calls]   # N, L, Ge, c, first chunk, second chunk, final
    calls = []
    for k, (n, L, Ge, c, c1, c2, final) in enumerate(cases):
        call = _Call(_dev(R.bursts(n)), L, Ge=Ge, c=c, rot=k)
        a, dst, plan = call.job(c1, False)
        LV.level_chunks([a])
        call.advance(plan)
        calls.append(call)
    singles, jobs = [], []
    for call, (n, L, Ge, c, c1, c2, final) in zip(calls, cases):
        a, dst, plan = call.job(c2, final)
        LV.level_chunks([a])
        singles.append(call.emitted(dst))
        jobs.append(call.job(c2, final))
    LV.level_chunks([j[0] for j in jobs])
    for k, (call, (a, dst, plan), want) in enumerate(zip(calls, jobs, singles)):
        got = call.emitted(dst)
        assert got.numel() > 0 and torch.equal(got.view(torch.int32), want.view(torch.int32)), f'call {k}'


def test_bad_arguments_are_refused():
    """The entry point checks every sample range on the host before it launches (no launch, an error)."""
    from cv2amd import lib as Lb, level as LV
    call = _Call(_dev(R.bursts(1000)), 120)

    def refused(change, n_new=500, final=False, text=None):
        a, dst, plan = call.job(n_new, final)
        change(a)
        with pytest.raises(Lb.Cv2Error) as e:
            LV.level_chunks([a])
        assert Lb.lib().cv2_last_error().decode() == str(e.value) and (text is None or text in str(e.value))
        assert torch.isnan(dst[0]).all(), 'nothing was launched'

    def more(a):
        a.n_emit += 1                                                          # one sample more than the look-ahead allows
        a.dst_cap += 1
    refused(more, text='looks ahead')
    refused(lambda a: setattr(a, 'dst_cap', a.n_emit - 1), text='do not fit')
    refused(lambda a: setattr(a, 'L', 241))
    refused(lambda a: setattr(a, 'L', 23))
    refused(lambda a: setattr(a, 'c', 1.5))
    refused(lambda a: setattr(a, 'c', 0.0))
    refused(lambda a: setattr(a, 'Ge', float('nan')))
    refused(lambda a: setattr(a, 'weights', None))
    refused(lambda a: setattr(a, 'n_final', 7))
    a, dst, plan = call.job(500, False)
    LV.level_chunks([a])
    call.advance(plan)

    def dropped(a):
        a.first += 1                                                           # the first sample read is said to be dropped
        a.n_tail -= 1
    refused(dropped, final=True, text='retained from')
    refused(lambda a: setattr(a, 'n_emit', a.n_emit + 1) or setattr(a, 'dst_cap', a.dst_cap + 1), final=True, text='beyond the signal')
    peak = torch.zeros(1, device='cuda')

    def target(a):
        a.peak, a.T = peak.data_ptr(), 0.5
    refused(target, final=False, text='whole signal')                          # a peak target on a chunk that is not the call's last
    a, dst, plan = call.job(500, True)                                         # in a batch: the offender is named, nothing is launched
    b, dst_b, _ = call.job(500, True)
    b.n0 += 1
    with pytest.raises(Lb.Cv2Error, match='call 1'):
        LV.level_chunks([a, b])
    assert torch.isnan(dst[0]).all() and torch.isnan(dst_b[0]).all()
    with pytest.raises(Lb.Cv2Error):
        Lb.check(Lb.lib().cv2_level_peak_batch(None, None, 1, None, None))
