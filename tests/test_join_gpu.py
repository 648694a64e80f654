"""cv2_wave_bounds and cv2_wave_join (csrc/join.hip) on the device, through the C ABI: the kept ranges equal the integers of the numpy
restatement (tests/_join.py) exactly, the joined signal equals it bit for bit, bad arguments are refused before anything is launched.
Sources and destinations sit at odd offsets inside NaN-guarded buffers.  Run with -m gpu."""
import numpy as np
import pytest
import torch

import _join as R

pytestmark = pytest.mark.gpu

GUARD = 9
LENGTHS = (1, 239, 240, 241, 1023, 1024, 1025, 4097, 24007)


def _guarded(x, off):
    """x (numpy float32) inside a larger device buffer, `off` floats past a 16-byte boundary, NaN around it -> (buffer, view)"""
    buf = torch.full((off + x.size + GUARD,), float('nan'), dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    buf[off:off + x.size] = torch.from_numpy(x)
    return buf, buf[off:off + x.size]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _speechlike(rng, n, lo, hi, level=0.5, floor=1e-4):
    """n samples: a low noise floor with a loud region [lo, hi)"""
    x = (rng.standard_normal(n) * floor).astype(np.float32)
    x[lo:hi] = (rng.standard_normal(hi - lo) * level).astype(np.float32)
    return x


def _bounds(segs, g, offs=None):
    from cv2amd import join as J
    offs = offs or [0] * len(segs)
    held = [_guarded(s, o) for s, o in zip(segs, offs)]
    b, p = J.wave_bounds([v for _, v in held], float(g))
    torch.cuda.synchronize()
    for (buf, _), s, o in zip(held, segs, offs):                              # the sources are read only
        assert torch.isnan(buf[:o]).all() and torch.isnan(buf[o + s.size:]).all()
    return [tuple(r) for r in b.cpu().tolist()], p.cpu().numpy()


def _check_bounds(segs, trim_db, offs=None):
    g = R.gain(trim_db)
    got, peaks = _bounds(segs, g, offs)
    assert got == R.bounds(segs, g), (trim_db, [s.size for s in segs])
    assert np.array_equal(peaks, np.array([R.peak(s) for s in segs], dtype=np.float32))
    return got


def test_bounds_every_length_and_source_alignment():
    rng = np.random.default_rng(11)
    for n in LENGTHS:                                                         # as the middle segment of three: both edges can be trimmed
        segs = []
        for i in range(3):
            m = n if i == 1 else 1500 + 7 * i
            lo = int(rng.integers(0, m))
            segs.append(_speechlike(rng, m, lo, int(rng.integers(lo, m)) + 1))
        for offs in ((0, 0, 0), (1, 2, 3), (3, 1, 2), (2, 3, 1)):
            _check_bounds(segs, 40, list(offs))
    # every length in ONE launch (k = 9), then k = 1 and k = 2
    segs = [_speechlike(rng, n, n // 3, n // 3 + max(1, n // 4)) for n in LENGTHS]
    got = _check_bounds(segs, 30, [i % 4 for i in range(len(segs))])
    assert got[0][0] == 0 and got[-1][1] == LENGTHS[-1]                       # the call's own start and end are never trimmed
    assert _check_bounds(segs[-1:], 30) == [(0, LENGTHS[-1])]
    _check_bounds(segs[-2:], 30, [3, 1])


def test_bounds_edge_cases():
    rng = np.random.default_rng(12)
    n = 240 * 40 + 100
    quiet = lambda: (rng.standard_normal(n) * 1e-5).astype(np.float32)        # noqa: E731
    outer = _speechlike(rng, 3000, 1000, 2000)
    # a loud region that starts on sample 0 of a frame, one that ends on a frame's last sample
    a = quiet()
    a[240 * 7:240 * 7 + 500] = 0.5
    b = quiet()
    b[240 * 9 + 17:240 * 12] = -0.5
    got = _check_bounds([outer, a, b, outer], 40)
    assert got[1] == (240 * 7 - 480, 240 * 10 + 480) and got[2] == (240 * 9 - 480, 240 * 12 + 480)
    # one sample more on either side moves the bound by a frame
    a[240 * 7 - 1] = 0.5
    b[240 * 12] = 0.5
    got = _check_bounds([outer, a, b, outer], 40)
    assert got[1][0] == 240 * 6 - 480 and got[2][1] == 240 * 13 + 480
    # a partial last frame that is the only loud one; a loud first frame (the clamp at 0) and last frame (the clamp at n)
    c = quiet()
    c[240 * 40 + 50] = 0.25
    d = quiet()
    d[3], d[n - 1] = 0.5, 0.5
    got = _check_bounds([outer, c, d, outer], 40)
    assert got[1] == (240 * 40 - 480, n) and got[2] == (0, n)
    # an all-zero segment is kept whole, as is one of NaN only
    z, nan = np.zeros(n, np.float32), np.full(700, np.nan, np.float32)
    got = _check_bounds([outer, z, nan, outer], 40)
    assert got[1] == (0, n) and got[2] == (0, 700)
    # NaN counts as 0 (the frame around it is not loud); a large finite value sets the peak
    e = quiet()
    e[240 * 3 + 5] = np.nan
    e[240 * 20 + 1] = np.float32(3.0e38)
    e[240 * 30] = np.float32(1.0e30)                                          # 1e30 < 3e38 * 1e-2: not loud at 40 dB
    got = _check_bounds([outer, e, outer], 40)
    assert got[1] == (240 * 20 - 480, 240 * 21 + 480)
    # a frame whose peak EQUALS thr is loud, the next float below is not
    for trim_db in (20, 37.5, 40, 60):
        g = R.gain(trim_db)
        thr = np.float32(np.float32(0.75) * g)
        f = np.zeros(n, np.float32)
        f[240 * 20 + 3] = 0.75
        f[240 * 5 + 100] = thr
        f[240 * 33 + 7] = np.nextafter(thr, np.float32(0))
        got = _check_bounds([outer, f, outer], trim_db)
        assert got[1] == (240 * 5 - 480, 240 * 21 + 480)


def _joined(segs, bnds, pause, F, src_offs=None, dst_off=0):
    from cv2amd import join as J
    k = len(segs)
    src_offs = src_offs or [0] * k
    held = [_guarded(s, o) for s, o in zip(segs, src_offs)]
    want_p, N, spans = R.plan([s.size for s in segs], bnds, pause, F)
    pieces = [(a, m, off, (J.FADE_IN if fi else 0) | (J.FADE_OUT if fo else 0)) for a, m, off, fi, fo in want_p]
    buf, dst = _guarded(np.zeros(N, np.float32), dst_off)
    dst.fill_(float('nan'))                                                   # the kernel writes every sample, gaps included
    out = J.wave_join([v for _, v in held], pieces, N, F, dst=dst)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    assert torch.isnan(buf[:dst_off]).all() and torch.isnan(buf[dst_off + N:]).all(), 'wrote outside [dst, dst + N)'
    want, _ = R.join(segs, bnds, pause, F)
    assert torch.equal(_bits(dst.cpu()), _bits(torch.from_numpy(want))), (pause, F, [s.size for s in segs])
    for (a, m, off, fi, fo) in want_p[:-1]:                                   # gaps: +0.0 exactly (bit pattern 0)
        assert int(_bits(dst[off + m:off + m + pause].cpu()).abs().sum()) == 0
    return dst.cpu().numpy(), spans


def test_join_pauses_fades_and_alignment():
    rng = np.random.default_rng(13)
    segs = [rng.standard_normal(n).astype(np.float32) for n in (2000, 1111, 3001, 700)]
    segs[1][5] = np.float32('-0.0')
    full = [(0, s.size) for s in segs]
    trimmed = [(0, 1800), (240, 1000), (480, 2900), (100, 700)]
    k = 0
    for pause in (0, 1, 3, 3600):
        for F in (0, 1, 120):
            for bnds in (full, trimmed):
                _joined(segs, bnds, pause, F, src_offs=[(k + i) % 4 for i in range(4)], dst_off=k % 4)
                k += 1
    # without a fade the result is torch.cat of the segments and zero blocks
    got, spans = _joined(segs, full, 3, 0, dst_off=2)
    want = np.concatenate([np.concatenate([s, np.zeros(3, np.float32)]) for s in segs])[:-3]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and spans[1] == (2003, 3114)
    # a piece with m < 2 F keeps its samples unfaded; one with m == 2 F fades over its whole length
    short = [segs[0], rng.standard_normal(239).astype(np.float32), rng.standard_normal(240).astype(np.float32), segs[3]]
    got, spans = _joined(short, [(0, s.size) for s in short], 7, 120, src_offs=[1, 2, 3, 0], dst_off=3)
    assert np.array_equal(got[spans[1][0]:spans[1][1]], short[1]) and not np.array_equal(got[spans[2][0]:spans[2][1]], short[2])
    # k = 1: a pure copy, whatever F says (no interior edge)
    for off in range(4):
        got, _ = _joined(segs[2:3], [(0, 3001)], 3600, 120, src_offs=[3 - off], dst_off=off)
        assert np.array_equal(got.view(np.int32), segs[2].view(np.int32))


def test_join_pieces_at_tile_edges():
    """pieces that start and end inside, on, and one past a 1024-output tile edge, for every destination alignment"""
    rng = np.random.default_rng(14)
    for dst_off in range(4):
        for edge in (1023, 1024, 1025, 2047, 2048, 2049):
            for pause in (0, 1, 5):
                n0 = edge - dst_off                                            # piece 0 ends on `edge` of the shifted tile grid, piece 1 starts `pause` later
                segs = [rng.standard_normal(n).astype(np.float32) for n in (n0, 1024, 1, 1023)]
                _joined(segs, [(0, s.size) for s in segs], pause, 0, src_offs=[1, 0, 2, 3], dst_off=dst_off)
                _joined(segs, [(0, n0), (3, 1024), (0, 1), (0, 1023)], pause, 2, src_offs=[0, 3, 1, 2], dst_off=dst_off)
    # many short pieces inside one tile (k = 9), and a long signal of many tiles
    segs = [rng.standard_normal(n).astype(np.float32) for n in (5, 1, 2, 300, 3, 4, 1, 7, 9)]
    _joined(segs, [(0, s.size) for s in segs], 2, 1, src_offs=[i % 4 for i in range(9)], dst_off=1)
    segs = [rng.standard_normal(n).astype(np.float32) for n in (24007, 48000, 4097)]
    _joined(segs, [(0, 23000), (960, 47000), (480, 4097)], 3600, 120, src_offs=[0, 0, 2], dst_off=0)


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from cv2amd import join as J, lib as L
    lib = L.lib()
    J._bind(lib)
    src = torch.arange(1000, dtype=torch.float32, device='cuda')
    dst = torch.full((4000,), 7.0, dtype=torch.float32, device='cuda')
    table = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    fade = J.fade_table_dev('cuda', 120)
    bounds = torch.full((4, 2), -5, dtype=torch.int32, device='cuda')
    peaks = torch.full((4,), -5.0, device='cuda')

    def piece(src_off, m, dst_off, flags=0, n_src=1000):
        return J.WavePiece(src.data_ptr(), n_src, src_off, m, dst_off, flags, 0)

    def join(pieces, k=None, F=0, n_dst=4000, ft=fade):
        arr = (J.WavePiece * max(1, len(pieces)))(*pieces)
        return lib.cv2_wave_join(arr, table.data_ptr(), len(pieces) if k is None else k, ft.data_ptr() if ft is not None else None, F,
                                 dst.data_ptr(), n_dst, L.stream_ptr())
    bad = {
        'k = 0': lambda: join([piece(0, 10, 0)], k=0),
        'k = 257': lambda: join([piece(0, 1, i) for i in range(257)]),
        'overlapping pieces': lambda: join([piece(0, 100, 0), piece(0, 100, 99)]),
        'pieces out of order': lambda: join([piece(0, 100, 500), piece(0, 100, 0)]),
        'a piece beyond its source': lambda: join([piece(901, 100, 0)]),
        'a negative source offset': lambda: join([piece(-1, 100, 0)]),
        'a piece beyond the destination': lambda: join([piece(0, 101, 3900)]),
        'a fade flag with m < 2 F': lambda: join([piece(0, 239, 0, J.FADE_OUT), piece(0, 500, 300)], F=120),
        'a fade without a table': lambda: join([piece(0, 500, 0, J.FADE_OUT), piece(0, 500, 600)], F=120, ft=None),
        'unknown fade flags': lambda: join([piece(0, 500, 0, 4)]),
        'F < 0': lambda: join([piece(0, 500, 0)], F=-1),
    }
    for name, call in bad.items():
        assert call() == -1, name
        assert b'cv2_wave_join' in lib.cv2_last_error(), name
    seg = (J.WaveSeg * 1)(J.WaveSeg(src.data_ptr(), 1000, 0))

    def bnd(arr, k, g):
        return lib.cv2_wave_bounds(arr, table.data_ptr(), k, g, bounds.data_ptr(), peaks.data_ptr(), L.stream_ptr())
    assert bnd(seg, 0, 0.01) == -1 and bnd(seg, 257, 0.01) == -1 and bnd(seg, 1, 0.0) == -1 and bnd(seg, 1, 1.5) == -1
    assert bnd((J.WaveSeg * 1)(J.WaveSeg(src.data_ptr(), 0, 0)), 1, 0.01) == -1
    assert bnd((J.WaveSeg * 1)(J.WaveSeg(src.data_ptr() + 2, 10, 0)), 1, 0.01) == -1
    assert b'cv2_wave_bounds' in lib.cv2_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((bounds == -5).all()) and bool((peaks == -5.0).all())      # nothing ran
    # the same records, valid: accepted
    J.wave_join([src, src], [(0, 100, 0, 0), (900, 100, 100, 0)], 200, 0, dst=dst[:200])
    torch.cuda.synchronize()
    assert torch.equal(dst[:200].cpu(), torch.cat([src[:100], src[900:]]).cpu()) and bool((dst[200:] == 7.0).all())
