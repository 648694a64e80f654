"""fp16 against bf16 flow operands on one box, in one process (the same inputs through FlowEngine(operands='bf16') and FlowEngine(operands='fp16')):
flow ms at the configs[1] shape (P = 255, the 250 tokens of tests/golden/fullsize.npz), at a configs[2]-like batch of 32 (FR P = 255 / DE P = 310,
N ~ U{150..500}) and for one chunk round of 8 streams (P = 255, the third chunk), each the median of >= 20 HIP-event-timed calls; the mel error
of each engine against the reference's own mel of fullsize.npz.  The JSON record is printed (last line) and, with --out FILE, written there.
  python tools/exp_flow_fp16.py [reps] [--out FILE]      (--one fp16: one configs[1] call of the fp16 engine only, for a kernel trace)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from cv2amd import synth            # noqa: E402
from cv2amd.flow import FlowEngine  # noqa: E402

dev = 'cuda:0'
gd = np.load(os.path.join(ROOT, 'tests', 'golden', 'fullsize.npz'))
inp = synth.synthetic_inputs(prompt_len=int(gd['prompt_len']))
one = dict(token=torch.from_numpy(gd['token']), prompt_token=inp['prompt_token'], prompt_feat=inp['prompt_feat'], embedding=inp['embedding'])
sd = synth.make_flow()

if '--one' in sys.argv:
    e = FlowEngine(sd, dev, max_utts=1, max_len=1100, operands=sys.argv[sys.argv.index('--one') + 1])
    e.inference_batch([one])
    torch.cuda.synchronize()
    sys.exit(0)

out_path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
pos = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] != '--out']
reps = int(pos[0]) if pos else 20


def med_ms(fn, reps):
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


g = torch.Generator().manual_seed(1986)
b32 = []
for b in range(32):
    P = 255 if b % 2 == 0 else 310
    n = int(torch.randint(150, 501, (1,), generator=g))
    x = synth.synthetic_inputs(seed=6000 + b, prompt_len=P)
    b32.append(dict(token=torch.randint(0, 6561, (1, n), generator=g, dtype=torch.int32), prompt_token=x['prompt_token'].to(dev),
                    prompt_feat=x['prompt_feat'].to(dev), embedding=x['embedding'].to(dev)))
streams = []
for s in range(8):
    x = synth.synthetic_inputs(seed=7000 + s, prompt_len=255)
    streams.append(dict(token=torch.randint(0, 6561, (1, 250), generator=g, dtype=torch.int32), prompt_token=x['prompt_token'].to(dev),
                        prompt_feat=x['prompt_feat'].to(dev), embedding=x['embedding'].to(dev)))

res = {'reps': reps}
ref = torch.from_numpy(gd['mel']).unsqueeze(0)
for ops in ('bf16', 'fp16', 'bf16', 'fp16'):                 # interleaved twice: drift on the box shows up as a difference between the passes
    e1 = FlowEngine(sd, dev, max_utts=1, max_len=1100, operands=ops)
    mel = e1.inference_batch([one])[0].cpu()
    r = res.setdefault(ops, {'b1_ms': [], 'b32_ms': [], 'chunk8_ms': []})
    r['mel_rel_max_vs_reference'] = float((mel - ref).abs().max() / ref.abs().max())
    r['mel_rel_mean_vs_reference'] = float((mel - ref).abs().mean() / ref.abs().mean())
    r['b1_ms'].append(med_ms(lambda: e1.inference_batch([one]), reps))
    del e1
    e32 = FlowEngine(sd, dev, max_utts=32, max_len=2 * (310 + 500) + 8, operands=ops)
    r['b32_ms'].append(med_ms(lambda: e32.inference_batch(b32), reps))
    # chunk round of 8 streams: the caches hold the first two chunks (P = 255 pads the first chunk to 45 tokens, then 25), the timed call
    # computes the third (token prefix 95 + look-ahead 3)
    caches = [e32.new_cache(2 * (255 + 250)) for _ in streams]
    for n in (45 + 3, 70 + 3):
        e32.inference_chunk_batch([dict(u, token=u['token'][:, :n]) for u in streams], caches, finalize=False)
    state = [(c.n_cached, c.gen) for c in caches]
    third = [dict(u, token=u['token'][:, :98]) for u in streams]

    def chunk_round():
        for c, (nc, gen) in zip(caches, state):
            c.n_cached, c.gen = nc, gen                     # the same round again (the generation flip makes it repeatable)
        e32.inference_chunk_batch(third, caches, finalize=False)
    r['chunk8_ms'].append(med_ms(chunk_round, reps))
    del e32, caches
    torch.cuda.synchronize()
    print(ops, {k: v for k, v in r.items()}, flush=True)
for ops in ('bf16', 'fp16'):
    for k in ('b1_ms', 'b32_ms', 'chunk8_ms'):
        res[ops][k + '_median_of_passes'] = statistics.median(res[ops][k])
res['fp16_over_bf16'] = {k: res['fp16'][k + '_median_of_passes'] / res['bf16'][k + '_median_of_passes'] for k in ('b1_ms', 'b32_ms', 'chunk8_ms')}
res['fp16_over_bf16']['mel_rel_max_vs_reference'] = res['fp16']['mel_rel_max_vs_reference'] / res['bf16']['mel_rel_max_vs_reference']
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res['fp16_over_bf16']))
print(json.dumps(res))
