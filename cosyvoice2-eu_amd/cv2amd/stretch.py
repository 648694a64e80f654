"""Host planner of the streaming time-stretch (speed != 1 with stream=True; DESIGN.md section 1, k_stretch in csrc/hift.hip).

The stretch is defined on the global frame index of a stream: with r = float32(speed), output frame j reads the source position
x = max(0, r (j + 0.5) - 0.5) and is w0 m[i0] + w1 m[i1], i0 = floor(x), i1 = min(i0 + 1, N_final - 1).  Before the final chunk frame j
can be emitted as soon as i0 + 1 <= n_available - 1; at the final chunk everything up to int(N_final / speed) is emitted.  This module
only counts: which frames a chunk emits and from which source frame on the call has to retain its input.  Its index arithmetic is
bit for bit the kernel's: r, j + 0.5 and x are numpy.float32, and x is the kernel's single fused multiply-add -- r (j + 0.5) - 0.5
rounded ONCE (the form torch's CPU interpolation and k_interp_linear evaluate too).  numpy has no fma: the product and the
subtraction are exact in float64 (24 + 24 significant bits, j < 2^23), so one rounding of that float64 to float32 is the fma.  A
plain float32 product, or a Python float r, would round differently and let the plan and the kernel disagree by a frame.  No GPU,
no torch.
"""
import numpy as np

SPEED_MIN, SPEED_MAX = 0.5, 2.0          # a 50-frame chunk then emits at least 24 frames: every chunk still feeds the vocoder
_F32_HALF, _F32_ZERO = np.float32(0.5), np.float32(0.0)


def check_speed(speed):
    if not SPEED_MIN <= speed <= SPEED_MAX:
        raise ValueError(f'streaming synthesis supports {SPEED_MIN} <= speed <= {SPEED_MAX}, got {speed}')


def src_pos(r, j):
    """x of output frame j, fp32 (r: numpy.float32)."""
    assert isinstance(r, np.float32) and 0 <= j < 1 << 23
    x = np.float32(np.float64(r) * np.float64(np.float32(j) + _F32_HALF) - 0.5)      # fma(r, j + 0.5, -0.5): exact in float64, rounded once
    return x if x > _F32_ZERO else _F32_ZERO


def src_index(r, j):
    """i0 = floor(x) of output frame j."""
    return int(src_pos(r, j))


class StretchState:
    """Per-call state: frames consumed and emitted, and the global index of the first input frame still retained (the retained
    tail is the frames first .. consumed - 1; the tensors themselves live with the scheduler)."""
    __slots__ = ('speed', 'r', 'consumed', 'emitted', 'first', 'final')

    def __init__(self, speed):
        self.speed, self.r = float(speed), np.float32(speed)
        self.consumed = self.emitted = self.first = 0
        self.final = False

    @property
    def n_tail(self):
        return self.consumed - self.first

    def commit(self, n_new, n_emit, first_needed, final=False):
        """The chunk planned by plan(state, n_new, final) has been launched."""
        self.consumed += n_new
        self.emitted += n_emit
        self.first = first_needed
        self.final = final


def plan(state, n_new, final):
    """-> (j0, n_emit, first_needed) for a chunk of n_new further input frames: the chunk emits the output frames j0 .. j0 + n_emit - 1;
    afterwards the input frames from first_needed on are retained (first_needed <= consumed + n_new: nothing is retained when the next
    output frame starts beyond the frames seen so far).  Does not change the state: see StretchState.commit."""
    if state.final:
        raise ValueError('stretch: the stream has had its final chunk')
    if n_new < 0:
        raise ValueError('stretch: n_new < 0')
    r, j0 = state.r, state.emitted
    n_avail = state.consumed + n_new
    if final:
        n_out = int(n_avail / state.speed)                                     # the reference's size rule (F.interpolate(size=int(T / speed)))
        if n_out < j0:
            # cannot happen when the final chunk brings a frame (speed <= 2): the frames emitted before it number < (N - 1.5) / r + 0.5
            raise ValueError(f'stretch: {j0} frames emitted, the stream ends at {n_out}: the final chunk brought no frame')
        return j0, n_out - j0, n_avail
    # frame j can go out when floor(x_j) + 1 <= n_avail - 1; x_j is monotonic in j.  Start from the real-valued estimate, settle in fp32.
    j = max(j0, int((n_avail - 0.5) / float(r) - 0.5))
    while src_index(r, j) + 1 <= n_avail - 1:
        j += 1
    while j > j0 and src_index(r, j - 1) + 1 > n_avail - 1:
        j -= 1
    return j0, j - j0, min(src_index(r, j), n_avail)
