"""The streaming time-stretch on the host: the definition (tests/_stretch.py) against torch's linear interpolation where the two
scales coincide, and the planner (cv2amd/stretch.py) over every length 1..400.  No GPU."""
import numpy as np
import pytest
import torch

import _stretch as R
from cv2amd import stretch as S


@pytest.mark.parametrize('speed', R.SPEEDS)
def test_definition_equals_interpolate_where_the_scales_coincide(speed):
    """N / speed integral: F.interpolate's scale N / int(N / speed) is float32(speed) itself, its sample grid is the stream's."""
    rng = np.random.default_rng(11)
    n_cases, worst = 0, 0.0
    for n in range(1, 401):
        q = n / speed
        if q != round(q):
            continue
        m = rng.standard_normal((3, n)).astype(np.float32)
        want = torch.nn.functional.interpolate(torch.from_numpy(m)[None], size=int(n / speed), mode='linear')[0].numpy()
        got = R.stretch(m, speed)
        assert got.shape == want.shape == (3, int(q))
        worst = max(worst, float(np.abs(got - want).max()))
        n_cases += 1
    print(f'speed {speed}: {n_cases} lengths, worst abs difference {worst:.3e}')
    assert n_cases >= 50
    assert worst <= 1e-6


def test_speed_one_is_the_identity():
    m = np.random.default_rng(1).standard_normal((2, 77)).astype(np.float32)
    assert np.array_equal(R.stretch(m, 1.0), m)


@pytest.mark.parametrize('speed', R.PLAN_SPEEDS)
def test_planner_counts_and_retention(speed):
    """Every N in 1..400, chunkings from one frame at a time to everything at once: the emitted counts sum to int(N / speed); no
    emitted frame reads an input frame that was dropped (or one that has not arrived); nothing emittable is held back; what the
    planner retains is what the next frame reads first."""
    rng = np.random.default_rng(int(speed * 10000))
    for n in range(1, 401):
        i0 = R.index0(speed, np.arange(R.n_out(n, speed) + 2))                 # first source frame of every output frame, from the definition
        for chunks in R.chunkings(n, rng):
            st, total = S.StretchState(speed), 0
            for k, n_new in enumerate(chunks):
                final = k == len(chunks) - 1
                j0, n_emit, first_needed = S.plan(st, n_new, final)
                n_avail = st.consumed + n_new
                assert j0 == total and n_emit >= 0
                if n_emit:
                    assert i0[j0] >= st.first, (n, chunks, k, 'reads a dropped frame')
                    if final:
                        assert i0[j0 + n_emit - 1] <= n_avail - 1
                    else:
                        assert i0[j0 + n_emit - 1] + 1 <= n_avail - 1, (n, chunks, k, 'reads a frame that has not arrived')
                if final:
                    assert j0 + n_emit == R.n_out(n, speed)
                else:
                    assert not i0[j0 + n_emit] + 1 <= n_avail - 1, (n, chunks, k, 'holds back an emittable frame')
                    assert st.first <= first_needed == min(i0[j0 + n_emit], n_avail)
                st.commit(n_new, n_emit, first_needed, final)
                total += n_emit
                assert st.consumed == n_avail and st.emitted == total and 0 <= st.n_tail <= n_avail
            assert total == R.n_out(n, speed), (n, chunks)


def test_planner_arithmetic_is_fp32():
    """The positions are numpy.float32 from end to end (a Python float would round r (j + 0.5) differently from the kernel)."""
    for speed in R.PLAN_SPEEDS:
        r = np.float32(speed)
        for j in (0, 1, 7, 399, 12345, (1 << 23) - 1):
            x = S.src_pos(r, j)
            assert isinstance(x, np.float32)
            assert x == R.positions(speed, [j])[0]


def test_speed_range():
    for ok in (0.5, 0.8, 1.0, 2.0):
        S.check_speed(ok)
    for bad in (0.4, 2.5, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            S.check_speed(bad)
    st = S.StretchState(1.25)
    S.plan(st, 10, True)
    st.commit(10, 8, 10, True)
    with pytest.raises(ValueError):
        S.plan(st, 5, False)
