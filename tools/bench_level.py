"""The output level stage (cv2amd.level.Level) against the same build with the level unset -- which is the path of a build
without the stage: python tools/bench_level.py [out.json] [--rounds R].  Interleaved rounds, medians with their spread:
  * first-chunk latency and chunk gap of 1 and of 8 concurrent streams (the held-back look-ahead, 5 ms of audio, is by construction; what is
    reported here is time);
  * the wall time of a 10 s non-streaming call without a level, with a gain under the ceiling, and with a peak target (one launch more);
  * the kernel time alone for 240 000 samples: the level launch at L = 24 / 120 / 240, and the peak launch, by device events over a loop.
Writes profiles/level.json."""
import json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import torch
from cv2amd import level as LV, synth
from cv2amd.level import Level
from cosyvoice.cli.model import CosyVoice2Model

_a = [x for i, x in enumerate(sys.argv[1:]) if not x.startswith('--') and sys.argv[i] != '--rounds']
OUT = _a[0] if _a else os.path.join(ROOT, 'profiles', 'level.json')
ROUNDS = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 5
N = 8
m = CosyVoice2Model(synth.make_llm(), synth.make_flow(), synth.make_hift(), max_text=128, max_prompt_tokens=320, max_new_tokens=1100, max_batch=N)
inp = synth.synthetic_inputs(seed=1986, text_len=12, prompt_len=255, prompt_text_len=20)
kw = dict(text=inp['text'], prompt_text=inp['prompt_text'], llm_prompt_speech_token=inp['prompt_token'],
          flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'], flow_embedding=inp['embedding'],
          llm_embedding=inp['embedding'])
LEVELS = {'unset': None, 'limiter': Level(ceiling_db=-1), 'peak target': Level(peak_db=-3)}


def med(xs):
    xs = sorted(xs)
    return dict(median_ms=round(statistics.median(xs) * 1e3, 3), min_ms=round(xs[0] * 1e3, 3), max_ms=round(xs[-1] * 1e3, 3), n=len(xs))


def streams(n, level):
    first, gaps = [None] * n, []
    t0 = time.perf_counter()

    def work(i):
        t_prev = None
        for _out in m.tts(**kw, stream=True, force_len=250, level=level):
            now = time.perf_counter()
            if first[i] is None:
                first[i] = now - t0
            else:
                gaps.append(now - t_prev)
            t_prev = now
    ths = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    return first, gaps


def whole(level):
    t0 = time.perf_counter()
    (o,) = list(m.tts(**kw, stream=False, force_len=250, level=level))
    dt = time.perf_counter() - t0
    assert o['tts_speech'].shape[1] == 240000
    return dt


def kernels():
    out, dev = {}, m.device
    x = (torch.randn(240000, device=dev) * 0.4).contiguous()
    reps = 200
    for L in (24, 120, 240):
        st, w, dst = LV.LevelState(L), LV.weight_table(dev, L), torch.empty(240000, device=dev)
        a = LV.level_args(st, 1.0, float(Level().resolve()[1]), None, x, dst, 0, 240000, True, w)
        LV.level_chunks([a])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            LV.level_chunks([a])
        e1.record()
        torch.cuda.synchronize()
        out[f'level_L{L}_us'] = round(e0.elapsed_time(e1) / reps * 1e3, 2)
    LV.level_peaks([x])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        LV.level_peaks([x])
    e1.record()
    torch.cuda.synchronize()
    out['peak_us_with_table_upload'] = round(e0.elapsed_time(e1) / reps * 1e3, 2)
    out['note'] = 'back-to-back launches over the same 240 000 samples (0.96 MB: cache-resident), host launch cost included where it exceeds the kernel'
    return out


res = {'shape': 'synthetic weights at the real shapes, prompt of 255 tokens, 250 speech tokens = 10 s', 'rounds': ROUNDS, 'streams': {}, 'whole_call': {}}
for n in (1, N):                                                              # warm-up (graphs, tables, prompt caches)
    for lv in (None, LEVELS['limiter']):
        streams(n, lv)
for lv in LEVELS.values():
    whole(lv)
for n in (1, N):
    acc = {k: ([], []) for k in ('unset', 'limiter')}
    for _ in range(ROUNDS):
        for k in acc:                                                         # interleaved: both settings see the same drift
            f, g = streams(n, LEVELS[k])
            acc[k][0].extend(f)
            acc[k][1].extend(g)
    res['streams'][str(n)] = {k: dict(first_chunk=med(f), chunk_gap=med(g)) for k, (f, g) in acc.items()}
acc = {k: [] for k in LEVELS}
for _ in range(ROUNDS + 2):
    for k in acc:
        acc[k].append(whole(LEVELS[k]))
res['whole_call'] = {k: med(v) for k, v in acc.items()}
res['kernels_240000_samples'] = kernels()
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
