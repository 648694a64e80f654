"""The oracle's two extra modes (oracle/llm.py: fp64, split_operands) and its teacher-forced trace, on the CPU.

The default fp32 mode is pinned by tests/test_oracle_golden.py; here the trace helper is tied to that mode bit for bit, the fp64
mode is held to the fp32 one (a dtype leak in it -- an fp32 softmax, an fp64 RoPE angle -- shows as a distance far above fp32
rounding), and the split-operand model is capped in absolute terms so that the ratio bars of tests/test_llm_logits_gpu.py
(HIP <= 1.5 x model) cannot hide a failure behind a bad model.  Distances: max / rms over the vocabulary of |delta logit|,
relative to the step's max |logit|, maximum over a prefill + 12 teacher-forced decode steps."""
import pytest
import torch

from _bars import bar
from _llm_trace import dist, oracle_traces, record

STEPS = 12


def _case(layers, heavy=False):
    from cv2amd import synth, weights as W
    from oracle import llm as OL
    sd = synth.make_llm(layers=layers)
    if heavy:
        sd = synth.heavy_tail_llm(sd)
    sdr = W.round_llm_sd(sd)
    inp = synth.synthetic_inputs(seed=11, text_len=7, prompt_len=21, prompt_text_len=3)
    x = OL.build_lm_input(sdr, inp['text'], inp['prompt_text'], inp['prompt_token'])
    t = OL.LogitTrace(sdr)                                    # the ids to feed: the fp32 oracle's own greedy walk
    lg, ids = t.feed(x), []
    for _ in range(STEPS):
        ids.append(int(lg[:OL.SPEECH_TOKEN_SIZE].argmax()))
        lg = t.step(ids[-1])
    return sdr, OL.to_fp64(sdr), x, ids


@pytest.fixture(scope='module')
def small():
    return _case(3)


def test_trace_is_the_default_mode_bit_for_bit(small):
    """logit_trace in the default mode == the step loop of `inference` (which the goldens pin): same log-probabilities, bit for bit."""
    from cv2amd import synth
    from oracle import llm as OL
    sdr = small[0]
    inp = synth.synthetic_inputs(seed=11, text_len=7, prompt_len=21, prompt_text_len=3)
    ids, logps = OL.inference(sdr, inp['text'], inp['prompt_text'], inp['prompt_token'], force_len=6, return_logp=True)
    tr = OL.logit_trace(sdr, small[2], ids[:5])
    assert tr.dtype == torch.float32
    for j, lp in enumerate(logps):
        want = tr[j].log_softmax(dim=-1)
        want[OL.SPEECH_TOKEN_SIZE:] = float('-inf')           # force_len masks EOS and the ids above it (inference())
        assert torch.equal(want, lp), f'step {j}'


def test_split_mode_leaves_nothing_switched_on(small):
    from oracle import llm as OL
    sdr, _, x, ids = small
    a = OL.logit_trace(sdr, x, ids[:2])
    with OL.split_operands():
        b = OL.logit_trace(sdr, x, ids[:2])
    assert not OL.SPLIT['on'] and torch.equal(a, OL.logit_trace(sdr, x, ids[:2])) and not torch.equal(a, b)


def _check(name, case, cap_model):
    sdr, sd64, x, ids = case
    ref, mod, f32 = oracle_traces(sdr, sd64, x, ids)
    assert ref.dtype == torch.float64 and mod.dtype == torch.float32 and f32.dtype == torch.float32
    (fm, fr), (mm, mr) = dist(f32, ref), dist(mod, ref)
    record('cpu ' + name, fp32_max=fm.max().item(), fp32_rms=fr.max().item(), model_max=mm.max().item(), model_rms=mr.max().item())
    print(f'{name}: fp32 {fm.max():.2e} / {fr.max():.2e}   split-operand model {mm.max():.2e} / {mr.max():.2e}')
    if cap_model:
        # 1e-5: ten times the fp32 oracle's measured distance from fp64 (6.2e-7 at 3 layers, 1.3e-6 at 24); a leak is 1e-4 and up
        bar(f'oracle fp32 vs fp64, {name} (rel to max logit)', fm.max().item(), 1e-5)
        # 2e-4: the project's prefill-logit bar; the model measures 5.6e-6 / 1.3e-5
        bar(f'oracle split-operand model vs fp64, {name} (rel to max logit)', mm.max().item(), 2e-4)
    assert mm.max() > fm.max()                                # the model really rounds something
    return fm, mm


def test_fp64_and_split_modes_3_layers(small):
    _check('3 layers, Gaussian', small, True)


def test_fp64_and_split_modes_24_layers():
    _check('24 layers, Gaussian', _case(24), True)


def test_split_mode_on_heavy_tailed_weights_is_recorded():
    """heavy_tail_llm: the model's own distance is ~3e-4 (massive activations); no absolute cap there, the value is recorded."""
    _check('24 layers, heavy_tail_llm', _case(24, heavy=True), False)
