"""Host side of the output rate / PCM16 conversion (output_sample_rate, pcm16; DESIGN.md section 1, k_out_resample in csrc/output.hip).

The conversion is defined on the global sample index of a call: with g = gcd(24000, R), down = 24000 / g, up = R / g and
K[up][klen], width = cv2amd.prompt._sinc_kernel(24000, R), output o = i up + p reads the source samples q = i down - width + j,
j = 0 .. klen - 1 (those inside the signal).  Before the final chunk o can be emitted as soon as its last tap has arrived,
i down - width + klen - 1 <= n_available - 1; the final chunk emits everything up to ceil(N up / down).  The planner below only
counts -- which outputs a chunk emits, from which source sample on the call retains its input -- in Python integers, the same
integers the kernel's entry point checks, so the two cannot disagree by a rounding.  No GPU and no torch for the planner; the kernel
tables (cached per device and rate) and the launch need both.  There is no CPU fallback.
"""
import ctypes as C
import math

MODEL_RATE = 24000
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
F32, PCM16 = 0, 1                          # CV2_OUT_F32, CV2_OUT_PCM16
_shapes, _tables = {}, {}


def check_rate(rate):
    if isinstance(rate, bool) or not isinstance(rate, int) or rate not in RATES:
        raise ValueError(f'output_sample_rate must be one of {RATES}, got {rate!r}')
    return rate


def filter_shape(rate):
    """-> (up, down, klen, width) of 24000 -> rate; at 24000 there is no filter: (1, 1, 1, 0), every sample is its own output."""
    check_rate(rate)
    if rate not in _shapes:
        if rate == MODEL_RATE:
            _shapes[rate] = (1, 1, 1, 0)
        else:
            g = math.gcd(MODEL_RATE, rate)
            down, up = MODEL_RATE // g, rate // g
            width = math.ceil(6 * down / (min(down, up) * 0.99))          # _sinc_kernel's width (lowpass_filter_width 6, rolloff 0.99)
            _shapes[rate] = (up, down, 2 * width + down, width)
    return _shapes[rate]


def n_out(n, rate):
    """samples a call of n 24 kHz samples yields at `rate`: ceil(n up / down), torchaudio's length rule"""
    up, down, _, _ = filter_shape(rate)
    return -(-n * up // down)


class OutState:
    """Per-call state: source samples consumed, outputs emitted, and the global index of the first source sample still retained
    (the retained tail is the samples first .. consumed - 1; the tensor itself lives with the scheduler)."""
    __slots__ = ('rate', 'up', 'down', 'klen', 'width', 'consumed', 'emitted', 'first', 'final')

    def __init__(self, rate):
        self.rate = check_rate(rate)
        self.up, self.down, self.klen, self.width = filter_shape(rate)
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
    """-> (o0, n_emit, first_needed) for a chunk of n_new further source samples: the chunk emits the outputs o0 .. o0 + n_emit - 1;
    afterwards the source samples from first_needed on are retained (fewer than klen + down).  Does not change the state: see
    OutState.commit."""
    if state.final:
        raise ValueError('outrate: the call has had its final chunk')
    if n_new < 0:
        raise ValueError('outrate: n_new < 0')
    up, down, klen, width = state.up, state.down, state.klen, state.width
    o0, n_avail = state.emitted, state.consumed + n_new
    if final:
        return o0, -(-n_avail * up // down) - o0, n_avail
    # i's last tap i down - width + klen - 1 has arrived for i <= i_max (floor division: -1 or less while none has); all `up` phases of i go together
    i_next = max((n_avail - klen + width) // down + 1, o0 // up, 0)
    return o0, i_next * up - o0, min(max(0, i_next * down - width), n_avail)


# ---- the device side -------------------------------------------------------------------------------------------------------------
class OutArgs(C.Structure):
    """cv2_out_args (80 bytes): one call's chunk."""
    _fields_ = [('tail', C.c_void_p), ('fresh', C.c_void_p), ('dst', C.c_void_p), ('kernel', C.c_void_p)] + [(n, C.c_int32) for n in
               ('first', 'n_tail', 'n_avail', 'n_final', 'o0', 'n_emit', 'up', 'down', 'klen', 'width', 'format', 'dst_cap')]


def _bind(lib):
    if getattr(lib, '_out_bound', False):
        return
    lib.cv2_out_resample.argtypes = [C.POINTER(OutArgs), C.c_void_p]
    lib.cv2_out_resample_batch.argtypes = [C.POINTER(OutArgs), C.c_void_p, C.c_int32, C.c_void_p]
    lib._out_bound = True


def kernel_table(device, rate):
    """K[up][klen] of 24000 -> rate on `device` (fp32, the table cv2_resample takes), cached per (device, rate); None at 24000."""
    import torch
    from .prompt import _sinc_kernel
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), check_rate(rate))
    if key not in _tables:
        if rate == MODEL_RATE:
            _tables[key] = None
        else:
            k, width, down, up = _sinc_kernel(MODEL_RATE, rate)
            assert (up, down, k.shape[1], width) == filter_shape(rate) and k.shape[0] == up
            _tables[key] = torch.from_numpy(k).contiguous().to(device)
    return _tables[key]


def out_args(state, tail, fresh, dst, o0, n_emit, final, table):
    """One call's record for out_resample: tail / fresh (1-D fp32 device tensors, None or empty: no such samples) are the source samples
    state.first .. state.consumed + len(fresh) - 1, dst (1-D float32 or int16 device tensor) receives the outputs o0 .. o0 + n_emit - 1.
    The integers come from plan(); the samples stay on the device."""
    import torch
    a = OutArgs()
    for t in (tail, fresh):
        assert t is None or (t.dim() == 1 and t.dtype == torch.float32 and (t.numel() <= 1 or t.stride(0) == 1))
    assert dst.dim() == 1 and dst.dtype in (torch.float32, torch.int16) and (dst.numel() <= 1 or dst.stride(0) == 1)
    a.n_tail = 0 if tail is None else tail.numel()
    assert a.n_tail == state.n_tail
    if a.n_tail:
        a.tail = tail.data_ptr()
    n_new = 0 if fresh is None else fresh.numel()
    if n_new:
        a.fresh = fresh.data_ptr()
    if dst.numel():
        a.dst = dst.data_ptr()
    a.kernel = None if table is None else table.data_ptr()
    a.first, a.n_avail = state.first, state.consumed + n_new
    a.n_final = a.n_avail if final else -1
    a.o0, a.n_emit, a.dst_cap = o0, n_emit, dst.numel()
    a.up, a.down, a.klen, a.width = state.up, state.down, state.klen, state.width
    a.format = PCM16 if dst.dtype == torch.int16 else F32
    return a


def out_resample(args, device=None):
    """The conversion of one or several calls' chunks on the current HIP stream: cv2_out_resample, or ONE cv2_out_resample_batch
    launch (gridDim.z = calls) fed by a device table of the records.  The caller keeps the tensors behind the records alive."""
    import torch
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    if len(args) == 1:
        L.check(lib.cv2_out_resample(C.byref(args[0]), L.stream_ptr()))
        return
    n = len(args)
    arr = (OutArgs * n)(*args)
    host = torch.empty(n * C.sizeof(OutArgs), dtype=torch.uint8, pin_memory=True)
    C.memmove(host.data_ptr(), arr, n * C.sizeof(OutArgs))
    table = host.to(device or torch.device('cuda', torch.cuda.current_device()), non_blocking=True)     # (pinned: ordered on the stream, the host goes on)
    L.check(lib.cv2_out_resample_batch(arr, table.data_ptr(), n, L.stream_ptr()))
