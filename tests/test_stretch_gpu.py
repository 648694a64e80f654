"""k_stretch (cv2_mel_stretch / cv2_mel_stretch_batch) on the device: chunk invariance bit for bit, the values against the numpy
restatement of the definition (tests/_stretch.py), the identity at speed 1, the batched form against single calls.  Run with -m gpu."""
import numpy as np
import pytest
import torch

import _stretch as R

pytestmark = pytest.mark.gpu

ROWS, COL = 80, 8
LENGTHS = (1, 2, 3, 49, 50, 51, 137)


def _ragged(n):
    rng, left, out = np.random.default_rng(n), n, []
    while left:
        k = int(rng.integers(1, min(left, 37) + 1))
        out.append(k)
        left -= k
    return out


def _chunkings(n):
    return {'all at once': [n], 'one frame at a time': [1] * n, '50-frame chunks': [50] * (n // 50) + ([n % 50] if n % 50 else []),
            'ragged': _ragged(n)}


class _Stream:
    """What the scheduler keeps per call: the planner's state and the retained frames -- here with leading dimensions that differ
    from the row lengths and NaN guard columns around every destination."""

    def __init__(self, src, speed):
        from cv2amd import stretch as S
        self.S, self.src, self.st, self.tail, self.pos = S, src, S.StretchState(speed), None, 0

    def job(self, n_new, final):
        """-> (record, destination buffer, plan) of the next chunk; nothing advances"""
        from cv2amd.hift import stretch_args
        fresh = self.src[:, :, self.pos:self.pos + n_new]                      # a slice of the longer buffer: ld = its row length
        j0, n_emit, first_needed = self.S.plan(self.st, n_new, final)
        dst = torch.full((1, ROWS, COL + n_emit + 5), float('nan'), device=self.src.device)
        a = stretch_args(self.tail, fresh, dst, COL, self.st.first, self.st.consumed + n_new, j0, n_emit, self.st.r, final)
        return a, dst, (n_new, n_emit, first_needed, final, fresh)

    def advance(self, plan):
        n_new, n_emit, first_needed, final, fresh = plan
        drop, nt = first_needed - self.st.first, self.st.n_tail
        both = fresh if self.tail is None else torch.cat([self.tail, fresh], dim=2)
        keep = both[:, :, drop:]
        wide = torch.full((1, ROWS, keep.shape[2] + 3), float('nan'), device=fresh.device)      # the tail's ld differs from its length too
        wide[:, :, :keep.shape[2]] = keep
        self.tail = wide[:, :, :keep.shape[2]]
        assert self.tail.shape[2] == self.st.consumed + n_new - first_needed and nt >= 0
        self.st.commit(n_new, n_emit, first_needed, final)
        self.pos += n_new

    @staticmethod
    def emitted(dst, n_emit):
        assert torch.isnan(dst[:, :, :COL]).all() and torch.isnan(dst[:, :, COL + n_emit:]).all(), 'wrote outside its columns'
        return dst[:, :, COL:COL + n_emit]


def _run(src, n, speed, chunks):
    from cv2amd.hift import mel_stretch
    s, outs = _Stream(src, speed), []
    for k, n_new in enumerate(chunks):
        a, dst, plan = s.job(n_new, k == len(chunks) - 1)
        mel_stretch([a], rows=ROWS)
        outs.append(_Stream.emitted(dst, plan[1]))
        s.advance(plan)
    return torch.cat(outs, dim=2)


@pytest.fixture(scope='module')
def frames():
    assert torch.cuda.is_available(), 'needs a GPU'
    g = torch.Generator().manual_seed(17)
    return {n: torch.randn(1, ROWS, n + 7, generator=g).cuda() for n in LENGTHS}      # 7 columns more than the stream is long


@pytest.mark.parametrize('speed', R.PLAN_SPEEDS)
@pytest.mark.parametrize('n', LENGTHS)
def test_chunk_invariance_and_values(frames, n, speed):
    src = frames[n]
    once = _run(src, n, speed, [n])
    assert once.shape == (1, ROWS, R.n_out(n, speed))
    for name, chunks in _chunkings(n).items():
        got = _run(src, n, speed, chunks)
        assert torch.equal(got, once), f'N={n} speed={speed}: "{name}" differs from the one-shot result'
    want, a, b = R.stretch(src[0, :, :n].cpu().numpy(), speed, with_operands=True)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
    err = np.abs(once[0].cpu().numpy().astype(np.float64) - want.astype(np.float64))
    worst = float((err / ulp).max()) if err.size else 0.0
    print(f'N={n} speed={speed}: worst error {worst:.2f} ulp of the larger operand')
    assert worst <= 2.0
    if speed == 1.0:
        assert torch.equal(once, src[:, :, :n])


def test_batched_equals_single_calls(frames):
    """3 streams of different N, speed and j0 (each has had a first chunk) in ONE launch against the three single calls."""
    from cv2amd.hift import mel_stretch
    cases = [(137, 0.8, 50, 50, False), (51, 1.25, 20, 31, True), (50, 2.0, 3, 40, False)]          # N, speed, first chunk, second chunk, final
    streams, jobs = [], []
    for n, speed, c1, c2, final in cases:
        s = _Stream(frames[n], speed)
        a, dst, plan = s.job(c1, False)
        mel_stretch([a], rows=ROWS)
        s.advance(plan)
        streams.append(s)
    singles, batched = [], []
    for s, (n, speed, c1, c2, final) in zip(streams, cases):
        a, dst, plan = s.job(c2, final)
        mel_stretch([a], rows=ROWS)
        singles.append(_Stream.emitted(dst, plan[1]))
        jobs.append(s.job(c2, final))
    assert len({j[0].j0 for j in jobs}) == 3 and all(j[0].j0 > 0 for j in jobs)
    mel_stretch([j[0] for j in jobs], rows=ROWS)
    for k, ((a, dst, plan), want) in enumerate(zip(jobs, singles)):
        got = _Stream.emitted(dst, plan[1])
        assert got.shape[2] > 0 and torch.equal(got, want), f'stream {k}'


def test_bad_arguments_are_refused(frames):
    """The entry point checks every frame range on the host before it launches (no launch, an error)."""
    from cv2amd import lib as L
    from cv2amd.hift import mel_stretch
    s = _Stream(frames[50], 1.25)
    a, dst, plan = s.job(50, False)
    a.n_emit += 1                                                              # one frame more than has arrived
    with pytest.raises(L.Cv2Error):
        mel_stretch([a], rows=ROWS)
    a, dst, plan = s.job(50, False)
    a.first += 1                                                               # the first frame read is said to be dropped
    with pytest.raises(L.Cv2Error):
        mel_stretch([a], rows=ROWS)
    a, dst, plan = s.job(50, False)
    a.dst_col = a.ld_dst - 1                                                   # does not fit the destination row
    with pytest.raises(L.Cv2Error):
        mel_stretch([a], rows=ROWS)
