"""k_out_resample (cv2_out_resample / cv2_out_resample_batch) on the device: chunk invariance bit for bit, bit equality with the
existing cv2_resample on the whole signal, the values against the fp64 restatement of the definition (tests/_outrate.py) within a
derived bound, the int16 rule, the batched form against single calls.  Run with -m gpu."""
import numpy as np
import pytest
import torch

import _outrate as R

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 9, 12345
DST_OFFS = (1, 3, 5, 7)            # element offsets of the destination in its 16-byte-aligned buffer: aligned to the element, never to 4 elements


def _guarded(x, off, dtype=torch.float32):
    """x inside a larger device buffer, `off` elements in, NaN (int16: a sentinel) around it -> (buffer, view)"""
    fill = SENTINEL if dtype == torch.int16 else float('nan')
    buf = torch.full((off + x.numel() + GUARD,), fill, dtype=dtype, device='cuda')
    buf[off:off + x.numel()] = x
    return buf, buf[off:off + x.numel()]


class _Call:
    """What the scheduler keeps per call: the planner's state and the retained samples -- here with the source, the tail and every
    destination at odd offsets inside guarded buffers."""

    def __init__(self, sig, rate, pcm=False):
        from cv2amd import outrate as O
        self.O, self.rate, self.pcm = O, rate, pcm
        self.src_buf, self.src = _guarded(sig, 7)
        self.st, self.tail, self.pos, self.k = O.OutState(rate), None, 0, 0
        self.table = O.kernel_table('cuda', rate)

    def job(self, n_new, final):
        """-> (record, destination buffer, plan) of the next chunk; nothing advances"""
        fresh = self.src[self.pos:self.pos + n_new]
        o0, n_emit, first_needed = self.O.plan(self.st, n_new, final)
        off = DST_OFFS[self.k % len(DST_OFFS)]
        dtype = torch.int16 if self.pcm else torch.float32
        buf, dst = _guarded(torch.zeros(n_emit, dtype=dtype, device='cuda'), off, dtype)
        dst.fill_(SENTINEL if self.pcm else float('nan'))
        a = self.O.out_args(self.st, self.tail, fresh, dst, o0, n_emit, final, self.table)
        return a, (buf, off, n_emit), (n_new, n_emit, first_needed, final, fresh)

    def advance(self, plan):
        n_new, n_emit, first_needed, final, fresh = plan
        both = fresh if self.tail is None else torch.cat([self.tail, fresh])
        keep = both[first_needed - self.st.first:]
        self.tail = _guarded(keep, 3)[1] if keep.numel() else None
        self.st.commit(n_new, n_emit, first_needed, final)
        self.pos += n_new
        self.k += 1

    def emitted(self, dst):
        buf, off, n_emit = dst
        if self.pcm:
            assert (buf[:off] == SENTINEL).all() and (buf[off + n_emit:] == SENTINEL).all(), 'wrote outside [dst, dst + n_emit)'
        else:
            assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + n_emit:]).all(), 'wrote outside [dst, dst + n_emit)'
        return buf[off:off + n_emit].clone()

    def guards_intact(self):
        return torch.isnan(self.src_buf[:7]).all() and torch.isnan(self.src_buf[7 + self.src.numel():]).all()


def _run(sig, rate, chunks, pcm=False):
    from cv2amd import outrate as O
    c, outs = _Call(sig, rate, pcm), []
    for k, n_new in enumerate(chunks):
        a, dst, plan = c.job(n_new, k == len(chunks) - 1)
        O.out_resample([a])
        outs.append(c.emitted(dst))
        c.advance(plan)
    assert c.guards_intact()
    return torch.cat(outs)


def _cv2_resample(sig, rate):
    """the existing kernel (csrc/frontend.hip) on the whole signal"""
    from cv2amd import lib as L, outrate as O
    from cv2amd import prompt
    lib = L.lib()
    prompt._bind(lib)
    up, down, klen, width = O.filter_shape(rate)
    x, k = sig.contiguous(), O.kernel_table('cuda', rate)
    out = torch.empty(R.n_out(x.numel(), rate), dtype=torch.float32, device='cuda')
    L.check(lib.cv2_resample(x.data_ptr(), x.numel(), k.data_ptr(), up, down, klen, width, out.data_ptr(), out.numel(), L.stream_ptr()))
    return out


@pytest.fixture(scope='module')
def signals():
    assert torch.cuda.is_available(), 'needs a GPU'
    return {n: torch.from_numpy(np.random.default_rng(n).standard_normal(n).astype(np.float32)).cuda() for n in R.LENGTHS}


@pytest.mark.parametrize('rate', R.RATES)
def test_chunk_invariance_and_values(signals, rate):
    _, up, down, klen, width = R.table(rate)
    for n in R.LENGTHS:
        sig = signals[n]
        once = _run(sig, rate, [n])
        assert once.shape == (R.n_out(n, rate),)
        for name, chunks in R.chunkings(n, one_by_one=n <= 257).items():
            got = _run(sig, rate, chunks)
            assert torch.equal(got, once), f'R={rate} N={n}: "{name}" differs from the one-shot result'
        if rate == 24000:
            assert torch.equal(once, sig)
            continue
        assert torch.equal(once, _cv2_resample(sig, rate)), f'R={rate} N={n}: differs from cv2_resample of the whole signal'
        # against fp64: an fmaf chain of <= klen terms rounds <= klen times, each by <= 2^-24 of a partial sum that is <= sum |K s|;
        # the bound of the definition, computed per sample
        y64, mag = R.resample64(sig.cpu().numpy(), rate, with_mag=True)
        err = np.abs(once.cpu().numpy().astype(np.float64) - y64)
        bound = (klen + 1) * 2.0 ** -24 * mag
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f'R={rate} N={n}: worst error {worst:.3f} of the bound')
        assert (err <= bound).all()


@pytest.mark.parametrize('rate', (8000, 16000, 24000, 44100))
def test_pcm16(signals, rate):
    from cv2amd import outrate as O
    seen = set()
    for n in (19, 42, 257, 1000):
        sig = (signals[n] * 0.4).contiguous()                                  # some samples beyond +-1: they saturate
        f = _run(sig, rate, [n])
        want = torch.from_numpy(R.pcm16(f.cpu().numpy()))
        for name, chunks in R.chunkings(n, one_by_one=False).items():
            c, outs = _Call(sig, rate, pcm=True), []
            for k, n_new in enumerate(chunks):
                a, dst, plan = c.job(n_new, k == len(chunks) - 1)
                O.out_resample([a])
                outs.append(c.emitted(dst))
                if a.n_emit:
                    seen.add((a.n_emit % 2, a.dst % 16))
                c.advance(plan)
            got = torch.cat(outs)
            assert got.dtype == torch.int16 and torch.equal(got.cpu(), want), f'R={rate} N={n} "{name}"'
    assert {p for p, _ in seen} == {0, 1}, 'odd and even n_emit'
    assert all(al % 4 == 2 for _, al in seen) and len({al for _, al in seen}) >= 3, 'destinations aligned to 2 bytes and to nothing more'


def test_pcm16_special_values():
    sp = [1.5, -1.5, 1.0, -1.0, -0.0, float('nan'), 0.5, -0.5, 32767 / 32768, 0.99999, -0.99999, 1e-6, 0.25]
    sig = torch.tensor(sp * 3, dtype=torch.float32).cuda()                     # 39 samples: odd n_emit; the chunkings below give even ones
    want = [32767, -32768, 32767, -32768, 0, 0, 16384, -16384, 32767, 32767, -32767, 0, 8192] * 3
    for chunks in ([39], [13, 26], [1, 2, 36], [4, 35]):
        assert _run(sig, 24000, chunks, pcm=True).tolist() == want, chunks
    f = _run(sig, 24000, [39])
    assert torch.equal(torch.nan_to_num(f, 7.0), torch.nan_to_num(sig, 7.0)) and torch.signbit(f[4])      # the pass-through is exact: -0.0 stays -0.0
    for rate in (16000, 44100):                                                # NaN spreads over the filter's support: those outputs are 0
        f = _run(sig, rate, [39])
        assert torch.isnan(f).any()
        assert torch.equal(_run(sig, rate, [20, 19], pcm=True).cpu(), torch.from_numpy(R.pcm16(f.cpu().numpy())))


@pytest.mark.parametrize('n_calls', (1, 3, 8))
def test_batched_equals_single_calls(signals, n_calls):
    """calls of different length, rate and format, each after a first chunk, in ONE launch against the single calls"""
    from cv2amd import outrate as O
    cases = [(4803, 16000, True, 480, 2000, False), (1000, 44100, False, 300, 700, True), (257, 8000, True, 100, 157, True),
             (4803, 48000, False, 2500, 2303, True), (1000, 24000, True, 1, 999, True), (256, 22050, False, 100, 150, False),
             (4803, 32000, True, 4000, 803, True), (42, 24000, False, 41, 1, True)][:n_calls]      # N, rate, pcm16, first chunk, second chunk, final
    calls = []
    for n, rate, pcm, c1, c2, final in cases:
        c = _Call(signals[n], rate, pcm)
        a, dst, plan = c.job(c1, False)
        O.out_resample([a])
        c.advance(plan)
        calls.append(c)
    singles, jobs = [], []
    for c, (n, rate, pcm, c1, c2, final) in zip(calls, cases):
        a, dst, plan = c.job(c2, final)
        O.out_resample([a])
        singles.append(c.emitted(dst))
        jobs.append(c.job(c2, final))
    O.out_resample([j[0] for j in jobs])
    for k, (c, (a, dst, plan), want) in enumerate(zip(calls, jobs, singles)):
        got = c.emitted(dst)
        assert got.numel() > 0 and got.dtype == want.dtype and torch.equal(got, want), f'call {k}'


def test_bad_arguments_are_refused(signals):
    """The entry point checks every sample range on the host before it launches (no launch, an error)."""
    from cv2amd import lib as L, outrate as O
    c = _Call(signals[1000], 16000)
    a, dst, plan = c.job(500, False)
    a.n_emit += 2                                                              # one output pair more than has arrived
    a.dst_cap += 2
    with pytest.raises(L.Cv2Error):
        O.out_resample([a])
    a, dst, plan = c.job(500, False)
    a.dst_cap = a.n_emit - 1                                                   # does not fit the destination
    with pytest.raises(L.Cv2Error):
        O.out_resample([a])
    a, dst, plan = c.job(500, False)
    O.out_resample([a])
    c.advance(plan)
    a, dst, plan = c.job(500, True)
    a.first += 1                                                               # the first sample read is said to be dropped
    a.n_tail -= 1
    with pytest.raises(L.Cv2Error):
        O.out_resample([a])
    a, dst, plan = c.job(500, True)
    a.down = 4000                                                              # a window no block can stage
    with pytest.raises(L.Cv2Error):
        O.out_resample([a])
