"""Fixture of the per-call flow solver tests (tests/test_solver_cpu.py, tests/test_solver_gpu.py): flow_solver.npz, the mel of flow_e2e.npz's
inputs (31 tokens, prompt 20, synth weights) from the REFERENCE's own CausalMaskedDiffWithXvec.inference under other solver settings:
decoder.inference_cfg_rate is set, and the decoder call is wrapped so that inference passes another n_timesteps (flow.py:278 writes 10).
Settings (steps, cfg_rate): (1, 0.7), (4, 0.7), (16, 0.7), (10, 0.0), (10, 1.5); tags full and stream_nonfinal; t_span of every step count.
The oracle (oracle.flow with the same settings, tests/_solver_oracle.py) must agree with the reference to 2e-5 before anything is written.
Needs the reference checkout (oracle/ref_harness.py).  ~1 min of CPU:  python tests/golden/make_golden_solver.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'cosyvoice2-eu_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from cv2amd import synth                 # noqa: E402
from oracle import ref_harness as R      # noqa: E402
from oracle import flow as OF            # noqa: E402
import _solver_oracle as SO              # noqa: E402


def gen_flow_solver():
    f = R.build_flow()
    sd = synth.make_flow()
    f.load_state_dict(sd, strict=True)
    gd = np.load(os.path.join(HERE, 'flow_e2e.npz'))
    P = int(gd['prompt_len'])
    inp = synth.synthetic_inputs(prompt_len=P)
    tok = torch.from_numpy(gd['token'])
    real_forward = f.decoder.forward
    out = {}
    for steps, cfg in SO.SETTINGS:
        f.decoder.inference_cfg_rate = cfg
        f.decoder.forward = lambda *a, n_timesteps=10, _n=steps, **k: real_forward(*a, n_timesteps=_n, **k)
        for tag, streaming, finalize in SO.TAGS:
            with torch.inference_mode():
                mr, _ = f.inference(token=tok, token_len=torch.tensor([tok.shape[1]]), prompt_token=inp['prompt_token'],
                                    prompt_token_len=torch.tensor([P]), prompt_feat=inp['prompt_feat'], prompt_feat_len=torch.tensor([2 * P]),
                                    embedding=inp['embedding'], streaming=streaming, finalize=finalize)
            mo = SO.inference(sd, tok, inp['prompt_token'], inp['prompt_feat'], inp['embedding'], streaming, finalize, steps, cfg)
            err = (mr - mo).abs().max().item()
            print(f'steps {steps} cfg {cfg} {tag}: oracle vs reference {err:.2e}')
            assert err < 2e-5, 'oracle != reference (flow solver settings)'
            out[SO.key(tag, steps, cfg)] = mr.numpy().astype(np.float32)
        out[f't_span_n{steps}'] = (1 - torch.cos(torch.linspace(0, 1, steps + 1) * 0.5 * torch.pi)).numpy()
        assert np.array_equal(out[f't_span_n{steps}'], OF.t_span(steps).numpy())
    if np.array_equal(out[SO.key('full', 10, 0.0)], out[SO.key('full', 10, 1.5)]):
        raise AssertionError('the guidance rate did not reach the reference')
    np.savez_compressed(os.path.join(HERE, 'flow_solver.npz'), settings=np.array(SO.SETTINGS, dtype=np.float64), **out)
    print('wrote flow_solver.npz', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    assert R.available(), 'needs the reference checkout'
    R.activate()
    gen_flow_solver()
