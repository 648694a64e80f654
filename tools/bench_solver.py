"""Flow stage against the call's Euler step count (cv2amd.solver.Solver), one process on an MI355X: flow ms of one utterance
at the configs[1] shape (P = 255, the 250 tokens of tests/golden/fullsize.npz) and of the flow call of a stream's FIRST chunk there (48 tokens behind the prompt,
chunk masks, not final; the flow call alone through FlowEngine.inference_batch, not the latency of a streaming tts() call), for steps in {4, 6, 10} and for the call without solver settings -- each the median of `reps` HIP-event-timed calls,
taken in `rounds` interleaved rounds whose medians' spread is reported beside them; and the first-chunk latency of a streaming tts() call with those
settings (tools/bench_stream.py's workload and clock: the call to the first yielded chunk, `reps` calls per setting, interleaved; median, min, p90).  The JSON record is printed (last line) and, with --out FILE,
written there.   python tools/bench_solver.py [reps] [rounds] [--out FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import time             # noqa: E402
import numpy as np      # noqa: E402
import torch            # noqa: E402
from cv2amd import synth            # noqa: E402
from cv2amd.flow import FlowEngine  # noqa: E402
from cv2amd.solver import Solver    # noqa: E402

out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] != '--out']
reps, rounds = (int(pos[0]) if pos else 20), (int(pos[1]) if len(pos) > 1 else 3)

dev = 'cuda:0'
gd = np.load(os.path.join(ROOT, 'tests', 'golden', 'fullsize.npz'))
P = int(gd['prompt_len'])
inp = synth.synthetic_inputs(prompt_len=P)
tok = torch.from_numpy(gd['token'])
first = 25 + (-(-P // 25) * 25 - P) + 3                                 # cli/model.py:353-357: hop + prompt pad + look-ahead
utt = {k: v.to(dev) for k, v in dict(token=tok, prompt_token=inp['prompt_token'], prompt_feat=inp['prompt_feat'], embedding=inp['embedding']).items()}
chunk = dict(utt, token=utt['token'][:, :first])
eng = FlowEngine(synth.make_flow(), dev, max_utts=1, max_len=1100)


def med_ms(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


legs = [('default', None)] + [(f'steps_{n}', Solver(steps=n)) for n in (4, 6, 10)]
res = {name: dict(flow_ms=[], flow_first_chunk_ms=[]) for name, _ in legs}
for _ in range(rounds):
    for name, sv in legs:
        kw = {} if sv is None else dict(solver=sv)
        res[name]['flow_ms'].append(med_ms(lambda: eng.inference_batch([utt], **kw)))
        res[name]['flow_first_chunk_ms'].append(med_ms(lambda: eng.inference_batch([chunk], streaming=True, finalize=False, **kw)))
rec = dict(shape=dict(prompt_tokens=P, tokens=int(tok.shape[1]), first_chunk_tokens=first), reps=reps, rounds=rounds, device=torch.cuda.get_device_name(0))
for name, r in res.items():
    rec[name] = {k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in r.items()}
# first-chunk latency through the scheduler: LLM prefill + 48 tokens + chunk-masked flow + HiFT on the first chunk's frames
del eng
from cosyvoice.cli.model import CosyVoice2Model    # noqa: E402
m = CosyVoice2Model(synth.make_llm(), synth.make_flow(), synth.make_hift(), max_text=128, max_prompt_tokens=320, max_new_tokens=1100)
si = synth.synthetic_inputs(text_len=50, prompt_len=255, prompt_text_len=20)
kw = dict(text=si['text'], flow_embedding=si['embedding'], llm_embedding=si['embedding'], prompt_text=si['prompt_text'],
          llm_prompt_speech_token=si['prompt_token'], flow_prompt_speech_token=si['prompt_token'], prompt_speech_feat=si['prompt_feat'])
lat = {name: [] for name, _ in legs}
for i in range(reps + 2):
    for name, sv in legs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = m.tts(**kw, stream=True, **({} if sv is None else dict(solver=sv)))
        next(g)
        t1 = time.perf_counter()
        g.close()
        if i >= 2:
            lat[name].append((t1 - t0) * 1e3)
for name, v in lat.items():
    rec[name]['tts_first_chunk_ms'] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), p90=round(float(np.percentile(v, 90)), 2))
line = json.dumps(rec)
if out_path:
    with open(out_path, 'w') as f:
        f.write(json.dumps(rec, indent=1) + '\n')
print(line)
