"""The loudness measurement on the device (csrc/loudness.hip) through the C ABI, against the float64 oracle of tests/_loudness.py: the block
grid at its edges, content on which both gates act, the high-pass's state hand-over between hops, non-finite samples, bit-for-bit invariance
to what shares the launch and to where the buffer lies, the gain path into cv2_level_chunk, and the argument checks.  Every input keeps the
oracle's gate margin (asserted).  Run with -m gpu.

Measured on an MI355X: the worst |Lk - oracle| over every case of this file and of test_loudness_api_gpu.py is R.WORST_LU; the bar R.BAR_LU
is 4 x that (never above 0.01 LU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _level as RL
import _loudness as R
from _bars import bar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = (0, 1, 9599, 9600, 9601, 11999, 12000, 12001, 24007, 73234)
_ref = {}


def _oracle(name, s):
    """the oracle's measure of a named input, computed once; the gate margin is a precondition of every comparison"""
    if name not in _ref:
        _ref[name] = R.measure(s)
        assert _ref[name]['margin'] >= R.MARGIN, f'{name}: gate margin {_ref[name]["margin"]:.4f} LU'
    return _ref[name]


def _measure(sigs, targets=None):
    from cv2amd import loudness as LD
    wavs = [s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s)).to(DEV) for s in sigs]
    Rr, lk = LD.measure(wavs, targets)
    torch.cuda.synchronize()
    return Rr.cpu().numpy(), lk.cpu().numpy()


def _hold(name, got, want):
    print(f'{name}: Lk {float(got)!r}, oracle {want!r}, apart {abs(float(got) - want):.3e} LU')
    bar(f'loudness_{name}', abs(float(got) - want), R.BAR_LU)


def test_block_grid_edges():
    sigs = [R.voice(73234, 21, amp=0.05)[:n] if n < 73234 else R.voice(73234, 21, amp=0.05) for n in LENGTHS]
    Rr, lk = _measure(sigs)
    for n, s, r, l in zip(LENGTHS, sigs, Rr, lk):
        m = _oracle(f'edge{n}', s)
        assert m['J'] == ((n - 9600) // 2400 + 1 if n >= 9600 else 0)
        if m['J'] == 0:
            assert r == 0.0 and l == -math.inf, n
        else:
            _hold(f'edge{n}', l, m['lufs'])
            assert abs(float(r) - math.sqrt(m['z'])) <= 2e-3 * math.sqrt(m['z'])


def test_content_against_the_oracle():
    bad, clean = R.specials()
    cases = {'bursts': R.bursts(), 'sine': R.sine(), 'rumble': R.rumble(), 'specials': bad, 'cleaned': clean,
             'silence': np.zeros(R.N_LONG, dtype=np.float32)}
    Rr, lk = _measure(list(cases.values()))
    got = dict(zip(cases, zip(Rr, lk)))
    b = _oracle('bursts', cases['bursts'])
    assert b['nB'] < b['nA'] < b['J'], 'both gates act'
    for name in ('bursts', 'sine', 'rumble', 'specials'):
        _hold(name, got[name][1], _oracle(name, cases[name])['lufs'])
    assert abs(_oracle('sine', cases['sine'])['lufs'] + 22.984) < 2e-3
    assert got['specials'][0].tobytes() == got['cleaned'][0].tobytes() and got['specials'][1].tobytes() == got['cleaned'][1].tobytes()
    assert got['silence'][0] == 0.0 and got['silence'][1] == -math.inf and _oracle('silence', cases['silence'])['lufs'] == -math.inf


def test_invariance_bit_for_bit():
    s = torch.from_numpy(R.bursts()).to(DEV)
    alone = _measure([s])
    others = [torch.from_numpy(R.voice(n, 30 + n % 7)).to(DEV) for n in (24007, 0, 9600, 73234 + 2400 * 5)]
    for pos in (0, 3, 6):
        batch = list(others[:2]) + list(others[2:]) + [others[0], others[3]]
        batch.insert(pos, s)
        assert len(batch) == 7 and any(b.numel() == 0 for b in batch)
        Rr, lk = _measure(batch)
        assert Rr[pos].tobytes() == alone[0][0].tobytes() and lk[pos].tobytes() == alone[1][0].tobytes(), pos
    base = torch.zeros(R.N_LONG + 64, dtype=torch.float32, device=DEV)
    off0 = (-(base.data_ptr() // 4)) % 4                                        # floats up to the next 16-byte boundary
    for k in range(4):
        view = base[off0 + k:off0 + k + R.N_LONG]
        assert (view.data_ptr() % 16) // 4 == k
        view.copy_(s)
        Rr, lk = _measure([view])
        assert Rr[0].tobytes() == alone[0][0].tobytes() and lk[0].tobytes() == alone[1][0].tobytes(), k
    again = _measure([s])
    assert again[0].tobytes() == alone[0].tobytes() and again[1].tobytes() == alone[1].tobytes()


def test_gain_path_into_the_level_kernel():
    from cv2amd import level as LV
    from cv2amd import loudness as LD
    lvl = LV.Level(loudness_lufs=-16)
    G, c, L, T = lvl.resolve()
    quiet, faint = R.voice(R.N_LONG, 8, amp=0.03), R.voice(R.N_LONG, 9, amp=2e-3)
    mq, mf = _oracle('quiet', quiet), _oracle('faint', faint)
    assert np.abs(quiet).max() * T / math.sqrt(mq['z']) < 0.9 * c and np.abs(faint).max() * 15.85 < 0.9 * c, 'the limiter stays idle'
    assert T / math.sqrt(mf['z']) > 1.5 * LD.G_MAX, 'far below the target'
    xs = [torch.from_numpy(v).to(DEV) for v in (quiet, faint)]
    Rr, lk = LD.measure(xs, [T, T])
    outs = []
    for i, x in enumerate(xs):
        st, dst = LV.LevelState(L), torch.empty_like(x)
        n0, n_emit, _first = LV.plan(st, x.numel(), True)
        LV.level_chunks([LV.level_args(st, G, c, None, x, dst, n0, n_emit, True, LV.weight_table(DEV, L), Rr[i:i + 1], T)])
        outs.append(dst)
    torch.cuda.synchronize()
    Rh = Rr.cpu().numpy()
    for name, s, r, y in (('quiet', quiet, Rh[0], outs[0]), ('faint', faint, Rh[1], outs[1])):
        ge = RL.gain(G, r, T)                                                   # fl(Ge * fl(T / R)) in numpy float32 from the device's R
        want = (ge * s).astype(np.float32)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32)), name
    _hold('quiet_in', lk[0].item(), mq['lufs'])
    out = R.measure(outs[0].cpu().numpy())
    assert out['margin'] >= R.MARGIN
    _hold('quiet_out', out['lufs'], -16.0)
    assert Rh[1] == np.float32(T) / np.float32(LD.G_MAX), 'the +24 dB clamp'
    assert abs(float(RL.gain(G, Rh[1], T)) / float(LD.G_MAX) - 1.0) < 3 * RL.U
    un, _ = _measure([xs[1]])                                                   # without a target R is sqrt(z) itself
    assert abs(float(un[0]) - math.sqrt(mf['z'])) <= 2e-3 * math.sqrt(mf['z'])


def test_argument_checks_launch_nothing():
    from cv2amd import lib as L
    from cv2amd import loudness as LD
    from cv2amd.level import WaveSeg, _upload
    lib = L.lib()
    LD._bind(lib)
    x = torch.from_numpy(R.sine(24007)).to(DEV)
    out = torch.full((2,), 7.0, dtype=torch.float32, device=DEV)
    filt, need = LD.filter_table(DEV), C.c_size_t(0)

    def call(arr, table, n, ws, ws_bytes):
        return lib.cv2_loudness_batch(arr, table, n, None, None, filt.data_ptr(), out[0:1].data_ptr(), out[1:2].data_ptr(), ws, ws_bytes, L.stream_ptr())
    good = (WaveSeg * 1)(WaveSeg(x.data_ptr(), x.numel(), 0))
    table = _upload(good, torch.device(DEV))
    assert lib.cv2_loudness_workspace_bytes(good, 1, C.byref(need)) == 0 and 10 * 9 * 4 <= need.value < 10 * 9 * 4 + 16
    ws = torch.empty(need.value // 4, dtype=torch.float32, device=DEV)
    neg = (WaveSeg * 1)(WaveSeg(x.data_ptr(), -5, 0))
    assert call(neg, table.data_ptr(), 1, ws.data_ptr(), need.value) == -1 and b'length' in lib.cv2_last_error()
    assert lib.cv2_loudness_workspace_bytes(neg, 1, C.byref(need)) == -1
    assert call(None, None, 1, ws.data_ptr(), need.value) == -1                 # a null table with n > 0
    assert call(good, None, 1, ws.data_ptr(), need.value) == -1
    assert call(good, table.data_ptr(), 1, ws.data_ptr(), 10 * 9 * 4 - 4) == -1 and b'workspace' in lib.cv2_last_error()
    assert call(good, table.data_ptr(), 1, None, 0) == -1
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0, 7.0], 'nothing was launched'
    assert call(good, table.data_ptr(), 1, ws.data_ptr(), need.value) == 0
    torch.cuda.synchronize()
    assert abs(out[1].item() - R.measure(R.sine(24007))['lufs']) < R.BAR_LU
