"""Per-call sampler settings and seeds without a GPU: the Sampling value's ranges, the float32 bit patterns of the
device record, the vocoder seed against its Philox definition, the .sampler() views and the C header."""
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')
HEADER = os.path.join(ROOT, 'include', 'cv2_amd.h')


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


@pytest.mark.parametrize('field,good,bad', [
    ('temperature', (0.05, 1, 1.7, 10), (0, 0.049, 10.5, -1, float('nan'), float('inf'), '1')),
    ('top_p', (1e-6, 0.3, 1, 1.0), (0, 0.0, 1.0001, -0.1, float('nan'))),
    ('top_k', (1, 5, 25), (0, 26, -1, 2.5, True)),
    ('win_size', (1, 10, 64), (0, 65, 1.5)),
    ('tau_r', (0, 0.0, 0.1, 7.5), (-1e-9, float('inf'), float('nan'))),
    ('seed', (0, 7, 2 ** 64 - 1), (-1, 2 ** 64, 1.0)),
    ('greedy', (True, False), (1, 0, 'yes')),
])
def test_check_ranges(field, good, bad):
    from cv2amd.sampling import Sampling
    for v in good:
        s = Sampling(**{field: v})
        assert s.check() is s and not s.is_default()
    for v in bad:
        with pytest.raises(ValueError):
            Sampling(**{field: v}).check()


def test_is_default_and_replace():
    from cv2amd.sampling import Sampling
    assert Sampling().is_default() and Sampling().check().is_default()
    assert Sampling(stream=3).is_default()                       # the segment index is not a setting
    for k, v in dict(seed=0, temperature=1.0, top_p=0.8, top_k=25, win_size=10, tau_r=0.1, greedy=False).items():
        assert not Sampling(**{k: v}).is_default(), k             # an explicit value equal to the default is still "set": it gets a record
    a = Sampling(seed=5, top_k=3)
    b = a.replace(top_k=7, temperature=None)
    assert (b.seed, b.top_k, b.temperature) == (5, 7, None) and a.top_k == 3
    c = a.for_segment(2)
    assert c.stream == 2 and a.stream == 0 and c.seed == 5


def test_record_packing_bit_patterns():
    """inv_temp = float32(1 / temperature); rep_thr = the fp32 product (float)win_size * (float)tau_r that cv2_llm_create forms; unset
    fields from the engine's constants"""
    import numpy as np
    from cv2amd.sampling import Sampling
    r = Sampling().record()
    assert r == dict(inv_temp=1.0, top_p=struct.unpack('<f', struct.pack('<f', 0.8))[0], top_k=25, win_size=10, rep_thr=1.0, stream=0)
    assert _bits(r['inv_temp']) == 0x3F800000 and _bits(r['rep_thr']) == 0x3F800000 and _bits(r['top_p']) == 0x3F4CCCCD
    for temp in (0.05, 0.5, 0.7, 1.0, 1.7, 3.0, 10):
        want = np.float32(1.0 / temp)
        assert _bits(Sampling(temperature=temp).record()['inv_temp']) == int(want.view(np.uint32)), temp
    for win, tau in ((10, 0.1), (16, 0.2), (64, 0.05), (7, 0.3), (33, 0.123456789), (1, 0.0)):
        want = np.float32(win) * np.float32(tau)
        assert isinstance(want, np.float32)
        assert _bits(Sampling(win_size=win, tau_r=tau).record()['rep_thr']) == int(want.view(np.uint32)), (win, tau)
    assert _bits(Sampling(win_size=16, tau_r=0.2).record()['rep_thr']) == _bits(3.2)
    # the engine's own constants fill what the call leaves unset
    r = Sampling(top_k=4, seed=9).record(dict(top_p=0.5, top_k=11, win_size=20, tau_r=0.25), stream=6)
    assert (r['top_p'], r['top_k'], r['win_size'], r['rep_thr'], r['stream'], r['inv_temp']) == (0.5, 4, 20, 5.0, 6, 1.0)
    assert Sampling(seed=1, stream=2).record()['stream'] == 2


def test_record_matches_the_ctypes_struct():
    import ctypes as C
    from cv2amd import lib as L
    from cv2amd.sampling import Sampling
    assert C.sizeof(L.LlmSampling) == 32
    assert [f[0] for f in L.LlmSampling._fields_] == ['inv_temp', 'top_p', 'top_k', 'win_size', 'rep_thr', 'stream', 'reserved']
    rec = Sampling(temperature=1.7, top_p=0.3, top_k=5, win_size=16, tau_r=0.2).record(stream=0xFFFFFFFF)
    s = L.LlmSampling(**rec)
    raw = struct.unpack('<ffiifIii', bytes(s))
    assert raw == (rec['inv_temp'], rec['top_p'], 5, 16, rec['rep_thr'], 0xFFFFFFFF, 0, 0)
    assert L.ST_SAMP == 15 and L.STATE_STRIDE == 16 and 'cv2_llm_set_sampling' in L.EXPORTS


def test_hift_seed_is_the_philox_definition():
    from cv2amd import philox
    from cv2amd.sampling import hift_seed
    seen = set()
    for seed in (0, 7, 0x1234ABCD5, 2 ** 64 - 1):
        for seg in (0, 1, 5):
            for chunk in (0, 1, 2, 40):
                r = philox.philox4x32((chunk, seg, 0x48694654, 0), (seed & 0xFFFFFFFF, seed >> 32))
                v = hift_seed(seed, seg, chunk)
                assert v == r[0] | (r[1] << 32) and 0 <= v < 2 ** 64
                seen.add(v)
    assert len(seen) == 4 * 3 * 4                                 # differs across seed, segment and chunk
    assert hift_seed(7, 1, 0) != hift_seed(7, 0, 1)


class _Model:
    """stands where CosyVoice2.model does: records what tts() was given"""

    def __init__(self):
        self.calls = []

    def tts(self, **kw):
        self.calls.append(kw)
        return iter(())


def _bare():
    from cosyvoice.cli.cosyvoice import CosyVoice2
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling = None, False, 24000, None
    cv.model, cv.frontend = _Model(), object()
    return cv


def test_sampler_view_shares_the_model_and_composes_with_output():
    from cv2amd.sampling import Sampling
    cv = _bare()
    v = cv.sampler(seed=7, temperature=0.5)
    assert v is not cv and v.model is cv.model and v.frontend is cv.frontend and cv.sampling is None
    assert v.sampling == Sampling(seed=7, temperature=0.5)
    w = v.output(sample_rate=16000, pcm16=True)
    assert w.sampling == v.sampling and w.output_sample_rate == 16000 and w.model is cv.model
    x = cv.output(sample_rate=8000).sampler(top_k=1)
    assert x.output_sample_rate == 8000 and x.sampling == Sampling(top_k=1)
    y = v.sampler(top_k=3)                                         # a view of a view keeps what it does not replace
    assert y.sampling == Sampling(seed=7, temperature=0.5, top_k=3) and v.sampling.top_k is None
    assert cv.sampler().sampling is None                           # nothing set: the model's sampler
    # _run hands the call's Sampling on, with the segment as its stream; nothing set -> no keyword at all
    list(y._run({}, False, 1.0, 'seg', 2))
    list(cv._run({}, False, 1.0, 'seg'))
    list(cv.sampler()._run({}, True, 1.0, 'seg', 1))
    got = cv.model.calls
    assert got[0]['sampling'] == Sampling(seed=7, temperature=0.5, top_k=3, stream=2) and got[0]['sampling'].stream == 2
    assert 'sampling' not in got[1] and 'sampling' not in got[2]


def test_bad_values_raise_before_the_model_is_touched():
    import inspect
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.model import CosyVoice2Model
    from cosyvoice2_eu import Cosy2EU
    from cv2amd.sampling import Sampling
    cv = _bare()
    for kw in (dict(top_k=26), dict(temperature=0), dict(top_p=0), dict(win_size=65), dict(tau_r=-1), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            cv.sampler(**kw)
        with pytest.raises(ValueError):
            Cosy2EU(cv).sampler(**kw)
    assert cv.model.calls == []
    # tts() itself refuses before any work: no attribute of the (unconstructed) model is reached
    mdl = CosyVoice2Model.__new__(CosyVoice2Model)
    with pytest.raises(ValueError):
        next(mdl.tts(sampling=Sampling(top_k=99)))
    names = list(inspect.signature(CosyVoice2Model.tts).parameters)
    assert names.index('sampling') > names.index('pcm16') and inspect.signature(CosyVoice2Model.tts).parameters['sampling'].default is None
    assert list(inspect.signature(CosyVoice2.sampler).parameters) == ['self', 'seed', 'temperature', 'top_p', 'top_k', 'win_size', 'tau_r', 'greedy']
    eu = Cosy2EU(cv).sampler(seed=3)
    assert isinstance(eu, Cosy2EU) and eu._model.model is cv.model and eu._model.sampling == Sampling(seed=3)


def test_llm_engine_methods_take_a_sampling():
    import inspect
    from cv2amd.llm import LLMEngine, BiStream
    for name in ('add_request', 'add_requests', 'generate', 'generate_fixed', 'new_bistream', 'bistream'):
        p = inspect.signature(getattr(LLMEngine, name)).parameters
        assert 'sampling' in p and p['sampling'].default is None, name
    assert 'sampling' in inspect.signature(BiStream.__init__).parameters


def test_header_declares_the_entry_point_and_keeps_the_abi():
    src = open(HEADER).read()
    assert re.search(r'#define\s+CV2_ABI_VERSION\s+3\b', src)
    assert re.search(r'CV2_ST_SAMP\s*=\s*15\b', src) and re.search(r'CV2_LLM_STATE_STRIDE\s*=\s*16\b', src)
    assert re.search(r'int\s+cv2_llm_set_sampling\s*\(\s*cv2_llm\s*\*\s*h\s*,\s*int32_t\s+slot\s*,\s*const\s+cv2_llm_sampling\s*\*', src)
    body = re.search(r'typedef struct \{([^}]*)\}\s*cv2_llm_sampling;', src).group(1)
    fields = re.findall(r'(float|int32_t|uint32_t)\s+(\w+)(\[2\])?;', body)
    assert [f[1] for f in fields] == ['inv_temp', 'top_p', 'top_k', 'win_size', 'rep_thr', 'stream', 'reserved']
    from cv2amd import lib as L
    assert L.ABI_VERSION == 3
