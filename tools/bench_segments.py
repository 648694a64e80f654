"""ONE caller reading a paragraph: 8 text segments of the configs[1] shape (P=255, 50 text tokens, 250 forced speech tokens = 10 s each)
on one CosyVoice2Model, synthetic weights at the real shapes.  Wall time, three repeats after a warm-up, of
  (a) the plain path: the 8 segments one after another, each a tts() call of its own (what inference_* does without .joined());
  (b) the joined call: CosyVoice2Model.tts_joined (150 ms pause, trim 40 dB: both new kernels and the copy of the bounds run);
  (c) the same 8 segments as 8 tts() calls from 8 threads (tools/bench_threads.py's pattern);
and, apart, the time of the join itself (cv2_wave_bounds + the copy of 2 k integers, cv2_wave_join) over 8 waveforms of 10 s, with every
piece on the 16-byte path and with an odd pause that puts every later piece on the per-sample path.
    python tools/bench_segments.py [out.json] [--parent parent.json]
(default: profiles/joined_segments.json; on a tree without tts_joined only (a), (c): run it there first and pass its file as --parent.)
Two conditions are stated in the file and decide the exit status: (b) is faster than (a) -- the parent's when given --, and (b) is not
slower than (c) by more than (c)'s spread plus the join's own time."""
import json, os, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import torch
from cv2amd import synth
from cosyvoice.cli.model import CosyVoice2Model

ARGS = sys.argv[1:]
PARENT = ARGS.pop(ARGS.index('--parent') + 1) if '--parent' in ARGS else None
ARGS = [a for a in ARGS if a != '--parent']
OUT = ARGS[0] if ARGS else os.path.join(ROOT, 'profiles', 'joined_segments.json')
K, N_TOK, REPEATS = 8, 250, 3
m = CosyVoice2Model(synth.make_llm(), synth.make_flow(), synth.make_hift(), max_text=128, max_prompt_tokens=320, max_new_tokens=1100, max_batch=8)
inps = [synth.synthetic_inputs(seed=1986 + i, text_len=50, prompt_len=255, prompt_text_len=20) for i in range(K)]
p0 = inps[0]                                                                  # one prompt, 8 texts
kws = [dict(text=inp['text'], prompt_text=p0['prompt_text'], llm_prompt_speech_token=p0['prompt_token'], flow_prompt_speech_token=p0['prompt_token'],
            prompt_speech_feat=p0['prompt_feat'], flow_embedding=p0['embedding'], llm_embedding=p0['embedding']) for inp in inps]


def plain():
    return sum(o['tts_speech'].shape[1] for kw in kws for o in m.tts(**kw, stream=False, force_len=N_TOK))


def threads():
    n = [0] * K

    def work(i):
        for o in m.tts(**kws[i], stream=False, force_len=N_TOK):
            n[i] += o['tts_speech'].shape[1]
    ths = [threading.Thread(target=work, args=(i,)) for i in range(K)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    return sum(n)


def joined():
    from cv2amd.join import Join
    (o,) = list(m.tts_joined(kws, Join(pause_ms=150, trim_db=40), force_len=N_TOK))
    return o['tts_speech'].shape[1]


def timed(fn):
    fn()                                                                      # warm-up (graphs, allocator)
    ts, b0 = [], len(m.batch_sizes)
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        ts.append(time.perf_counter() - t0)
    return {'wall_s': [round(t, 4) for t in ts], 'median_s': round(sorted(ts)[len(ts) // 2], 4), 'spread_s': round(max(ts) - min(ts), 4),
            'samples': n, 'audio_s_per_s': round(K * N_TOK * 960 / 24000.0 / sorted(ts)[len(ts) // 2], 1), 'batch_sizes': m.batch_sizes[b0:]}


def join_alone():
    """host-to-host time of the join's own work on 8 waveforms of 10 s: the bounds with their copy, and the join launch -- with the default
    pause (every piece congruent to the destination modulo 16 bytes: 16-byte loads and stores) and with a pause of 3601 samples (the
    pieces after the first fall off that congruence: per-sample loads)"""
    from cv2amd import join as J
    j = J.Join(pause_ms=150, trim_db=40)
    pause, F, g = j.resolve()
    odd = J.Join(pause_ms=3601 / 24, trim_db=40)
    assert odd.resolve()[0] == 3601
    wavs = [torch.randn(1, N_TOK * 960, device=m.device) * 0.1 for _ in range(K)]
    res = {'bounds_and_copy_s': [], 'join_s': [], 'join_unaligned_s': []}
    for _ in range(REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bounds = J.wave_bounds(wavs, g)[0].cpu().tolist()
        t1 = time.perf_counter()
        pieces, N, _ = J.plan([w.shape[1] for w in wavs], bounds, j)
        J.wave_join(wavs, pieces, N, F)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        pieces, N, _ = J.plan([w.shape[1] for w in wavs], bounds, odd)
        J.wave_join(wavs, pieces, N, F)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        res['bounds_and_copy_s'].append(round(t1 - t0, 6))
        res['join_s'].append(round(t2 - t1, 6))
        res['join_unaligned_s'].append(round(t3 - t2, 6))
    return {k: v[1:] for k, v in res.items()}                                 # (the first pass warms the tables)


res = {'workload': f'{K} segments, P=255, 50 text tokens, {N_TOK} forced speech tokens each, max_batch=8, non-streaming, synthetic weights; '
                   f'{REPEATS} repeats after a warm-up', 'device': torch.cuda.get_device_name(0)}
res['a_plain_sequential'] = timed(plain)
res['c_threads'] = timed(threads)
ok = True
if hasattr(m, 'tts_joined'):
    res['b_joined'] = timed(joined)
    res['join_alone'] = ja = join_alone()
    a = res['a_plain_sequential']
    if PARENT:
        with open(PARENT) as f:
            res['parent_commit'] = {k: v for k, v in json.load(f).items() if k in ('a_plain_sequential', 'c_threads')}
        a = res['parent_commit']['a_plain_sequential']
    b, c = res['b_joined'], res['c_threads']
    own = max(ja['bounds_and_copy_s']) + max(ja['join_s'])
    res['a_over_b'] = round(a['median_s'] / b['median_s'], 2)
    res['b_minus_c_s'] = round(b['median_s'] - c['median_s'], 4)
    res['conditions'] = {'a_is': 'parent commit' if PARENT else 'this tree', 'b_faster_than_a': b['median_s'] < a['median_s'],
                         'allowance_s': round(c['spread_s'] + own, 4), 'b_within_c_plus_allowance': res['b_minus_c_s'] <= c['spread_s'] + own}
    ok = res['conditions']['b_faster_than_a'] and res['conditions']['b_within_c_plus_allowance']
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
sys.exit(0 if ok else 1)
