"""ONE caller reading a paragraph aloud: 8 text segments of the configs[1] shape (P=255, 50 text tokens, 250 forced speech tokens = 10 s
each) streamed from one CosyVoice2Model, synthetic weights at the real shapes.  Three repeats after a warm-up, medians with the spread, of
  (a) the plain path: the 8 segments as 8 tts(stream=True) calls one after another (what inference_* does without .continuous());
  (b) the continuous call: CosyVoice2Model.tts_continuous (150 ms pause, trim 40 dB: both kernels and the record copy run);
each timed as: call -> first chunk, call -> last chunk, and the largest gap between a segment's last chunk and the next segment's first;
and, apart, (c) the added work of one chunk round -- gate, the copy of the four-integer record, emit -- on a 1 s chunk of a middle segment,
host to host, beside (d) what a plain stream pays to bring the same chunk to the host.
    python tools/bench_continuous.py [out.json] [--parent parent.json]
(default: profiles/continuous_stream.json; on a tree without tts_continuous only (a): run it there first and pass its file as --parent.)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import torch
from cv2amd import synth
from cosyvoice.cli.model import CosyVoice2Model

ARGS = sys.argv[1:]
PARENT = ARGS.pop(ARGS.index('--parent') + 1) if '--parent' in ARGS else None
ARGS = [a for a in ARGS if a != '--parent']
OUT = ARGS[0] if ARGS else os.path.join(ROOT, 'profiles', 'continuous_stream.json')
K, N_TOK, REPEATS = 8, 250, 3
m = CosyVoice2Model(synth.make_llm(), synth.make_flow(), synth.make_hift(), max_text=128, max_prompt_tokens=320, max_new_tokens=1100, max_batch=8)
inps = [synth.synthetic_inputs(seed=1986 + i, text_len=50, prompt_len=255, prompt_text_len=20) for i in range(K)]
p0 = inps[0]                                                                  # one prompt, 8 texts
kws = [dict(text=inp['text'], prompt_text=p0['prompt_text'], llm_prompt_speech_token=p0['prompt_token'], flow_prompt_speech_token=p0['prompt_token'],
            prompt_speech_feat=p0['prompt_feat'], flow_embedding=p0['embedding'], llm_embedding=p0['embedding']) for inp in inps]


def plain():
    """-> [(segment, time of the chunk)]"""
    ev = []
    for i, kw in enumerate(kws):
        for _o in m.tts(**kw, stream=True, force_len=N_TOK):
            ev.append((i, time.perf_counter()))
    return ev


def continuous():
    from cv2amd.join import Join
    return [(o['segment'], time.perf_counter()) for o in m.tts_continuous(kws, Join(pause_ms=150, trim_db=40), force_len=N_TOK)]


def timed(fn):
    fn()                                                                      # warm-up (graphs, allocator, prompt cache)
    runs = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = fn()
        seams = [t - ev[j - 1][1] for j, (i, t) in enumerate(ev) if j > 0 and i != ev[j - 1][0]]
        runs.append((ev[0][1] - t0, ev[-1][1] - t0, max(seams), len(ev)))

    def stat(c):
        v = sorted(r[c] for r in runs)
        return {'median_ms': round(v[len(v) // 2] * 1e3, 2), 'spread_ms': round((v[-1] - v[0]) * 1e3, 2)}
    return {'first_chunk': stat(0), 'last_chunk': stat(1), 'largest_seam_gap': stat(2), 'chunks': runs[0][3]}


def chunk_round_alone():
    """gate + record copy + emit of one 24 000-sample chunk in the middle of a middle segment (speech throughout: everything but the last
    120 samples goes out, they and the frame phase stay held), against the plain stream's copy of the same chunk to the host"""
    from cv2amd import join as J
    ws = J.WaveStream(J.Join(pause_ms=150, trim_db=40), 3, m.device)
    x = torch.randn(1, 24000, device=m.device) * 0.1
    ws.chunk(x, True)                                                         # segment 0, whole
    res = {'gate_copy_emit_us': [], 'plain_copy_to_host_us': [], 'with_copy_to_host_us': []}
    for _ in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = ws.chunk(x, False)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        o.cpu()
        t2 = time.perf_counter()
        x.cpu()
        t3 = time.perf_counter()
        res['gate_copy_emit_us'].append(round((t1 - t0) * 1e6, 1))
        res['with_copy_to_host_us'].append(round((t2 - t0) * 1e6, 1))
        res['plain_copy_to_host_us'].append(round((t3 - t2) * 1e6, 1))
    out = {k: {'median': sorted(v[2:])[len(v[2:]) // 2], 'min': min(v[2:]), 'max': max(v[2:])} for k, v in res.items()}
    out['launches_per_chunk'] = 2
    ws.close()
    return out


res = {'workload': f'{K} segments, P=255, 50 text tokens, {N_TOK} forced speech tokens each, one caller, stream=True, synthetic weights; '
                   f'{REPEATS} repeats after a warm-up', 'device': torch.cuda.get_device_name(0)}
res['a_plain_streams_in_sequence'] = timed(plain)
if hasattr(m, 'tts_continuous'):
    res['b_continuous'] = timed(continuous)
    res['chunk_round_alone'] = chunk_round_alone()
    if PARENT:
        with open(PARENT) as f:
            res['parent_commit'] = {k: v for k, v in json.load(f).items() if k == 'a_plain_streams_in_sequence'}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
