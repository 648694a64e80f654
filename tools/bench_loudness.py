"""The loudness target (Level(loudness_lufs=)) against the same build with no level set -- which is the path of a build without
the measurement: python tools/bench_loudness.py [out.json] [--rounds R].  Interleaved rounds, medians with their spread:
  * the measurement enqueue alone (cv2_loudness_batch: two passes, scan, finish, with its table uploads) over 10 s of audio and over
    32 x 10 s in one enqueue, by device events over a loop;
  * the wall time of a 10 s non-streaming call without a level, with a peak target and with a loudness target.
Writes profiles/loudness.json."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import torch
from cv2amd import loudness as LD, synth
from cv2amd.level import Level
from cosyvoice.cli.model import CosyVoice2Model

_a = [x for i, x in enumerate(sys.argv[1:]) if not x.startswith('--') and sys.argv[i] != '--rounds']
OUT = _a[0] if _a else os.path.join(ROOT, 'profiles', 'loudness.json')
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
m = CosyVoice2Model(synth.make_llm(), synth.make_flow(), synth.make_hift(), max_text=128, max_prompt_tokens=320, max_new_tokens=1100, max_batch=8)
inp = synth.synthetic_inputs(seed=1986, text_len=12, prompt_len=255, prompt_text_len=20)
kw = dict(text=inp['text'], prompt_text=inp['prompt_text'], llm_prompt_speech_token=inp['prompt_token'],
          flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'], flow_embedding=inp['embedding'],
          llm_embedding=inp['embedding'])
LEVELS = {'unset': None, 'peak target': Level(peak_db=-3), 'loudness target': Level(loudness_lufs=-16)}


def med(xs, unit='ms', scale=1e3):
    xs = sorted(xs)
    return {f'median_{unit}': round(statistics.median(xs) * scale, 3), f'min_{unit}': round(xs[0] * scale, 3), f'max_{unit}': round(xs[-1] * scale, 3), 'n': len(xs)}


def whole(level):
    t0 = time.perf_counter()
    (o,) = list(m.tts(**kw, stream=False, force_len=250, level=level))
    dt = time.perf_counter() - t0
    assert o['tts_speech'].shape[1] == 240000 and ('loudness_lufs' in o) == (level is not None and level.loud)
    return dt


def enqueue(k, reps=100):
    """ms per measurement of k signals of 240 000 samples, device events round `reps` enqueues"""
    xs = [(torch.randn(240000, device=m.device) * 0.1).contiguous() for _ in range(k)]
    tg = [LD.target(-16)] * k
    LD.measure(xs, tg)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        LD.measure(xs, tg)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


res = {'shape': 'synthetic weights at the real shapes, prompt of 255 tokens, 250 speech tokens = 10 s', 'rounds': ROUNDS}
for lv in LEVELS.values():                                                    # warm-up
    whole(lv)
acc = {k: [] for k in LEVELS}
for _ in range(ROUNDS + 2):
    for k in acc:                                                             # interleaved: every setting sees the same drift
        acc[k].append(whole(LEVELS[k]))
res['whole_call'] = {k: med(v) for k, v in acc.items()}
res['measurement_enqueue'] = {f'{k} x 240000 samples': med([enqueue(k) for _ in range(ROUNDS)], 'us', 1e6) for k in (1, 32)}
res['measurement_enqueue']['note'] = ('back-to-back enqueues over the same signals (cache-resident), each with the upload of its record '
                                      'table and the allocation of its workspace: the host cost is included where it exceeds the kernels')
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
