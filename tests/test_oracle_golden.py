"""oracle/ (CPU restatement) against the golden vectors captured from the real reference (tests/golden/make_golden.py)."""
import numpy as np
import pytest
import torch

from cv2amd import synth
from oracle import flow as OF
from oracle import hift as OH
from oracle import llm as OL


@pytest.fixture(scope='module')
def flow_sd():
    return synth.make_flow()


def _hift_noise(seed, T):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 9, generator=g), torch.randn(1, 480 * T, 9, generator=g)


@pytest.fixture
def golden_threads():
    """The hift goldens were captured with 8 torch threads.  The CPU kernels split their fp32 reductions by the thread count, so the last
    bits follow it (1, 2, 4, 6, 12 and 16 threads all differ from 8): the bit-exact comparison runs at 8 whatever the host's core count.
    A host whose BLAS picks other kernels (an AMD EPYC: ~1e-5 off at every thread count) cannot reproduce the goldens bit for bit."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize('name,T', [('hift_T24.npz', 24), ('hift_T16_cache.npz', 16)])
def test_hift_inference(golden, name, T, golden_threads):
    gd = golden(name)
    sd = synth.make_hift()
    ri, nz = _hift_noise(int(gd['noise_seed']), T)
    mel = torch.from_numpy(gd['mel'])
    assert torch.equal(OH.f0_predictor(sd, mel), torch.from_numpy(gd['f0']))
    wav, src = OH.inference(sd, mel, torch.from_numpy(gd['cache_source']), ri, nz)
    # bit-exact: same torch CPU ops in the same order as the reference
    assert torch.equal(src, torch.from_numpy(gd['source']))
    assert torch.equal(wav, torch.from_numpy(gd['wav']))


def test_flow_constants(golden):
    gd = golden('flow_e2e.npz')
    assert np.array_equal(OF.rand_noise()[0, 0, :16].numpy(), gd['rand_noise_head'])
    assert np.allclose(OF.t_span(10).numpy(), gd['t_span'], atol=0)


@pytest.mark.parametrize('tag,streaming,finalize', [('full', False, True), ('stream', True, True),
                                                    ('stream_nonfinal', True, False)])
def test_flow_e2e(golden, flow_sd, tag, streaming, finalize):
    gd = golden('flow_e2e.npz')
    inp = synth.synthetic_inputs(prompt_len=int(gd['prompt_len']))
    mel = OF.inference(flow_sd, torch.from_numpy(gd['token']), inp['prompt_token'], inp['prompt_feat'],
                       inp['embedding'], streaming, finalize)
    ref = torch.from_numpy(gd['mel_' + tag])
    assert mel.shape == ref.shape
    assert (mel - ref).abs().max() < 2e-5        # fp32 rounding only (explicit softmax vs SDPA)


@pytest.mark.parametrize('T', [16, 50, 101])
@pytest.mark.parametrize('tag,streaming', [('full', False), ('chunk', True)])
def test_flow_estimator(golden, flow_sd, T, tag, streaming):
    gd = golden('flow_estimator.npz')
    g = torch.Generator().manual_seed(100 + T)
    x = torch.randn(2, 80, T, generator=g)
    mu = torch.randn(2, 80, T, generator=g)
    mu[1] = 0
    cond = torch.randn(2, 80, T, generator=g)
    cond[1] = 0
    spks = torch.randn(2, 80, generator=g)
    spks[1] = 0
    y = OF.estimator(flow_sd, x, torch.ones(2, 1, T), mu, torch.full((2,), 0.3), spks, cond, streaming)
    assert (y - torch.from_numpy(gd[f'y_T{T}_{tag}'])).abs().max() < 2e-5


@pytest.mark.parametrize('T', [28, 53])
def test_flow_encoder(golden, flow_sd, T):
    gd = golden('flow_encoder.npz')
    g = torch.Generator().manual_seed(200 + T)
    xs = torch.randn(1, T, 512, generator=g)
    ctx = torch.randn(1, 3, 512, generator=g)
    for tag, streaming, c in (('full', False, None), ('chunk', True, None), ('chunk_ctx', True, ctx)):
        h = OF.encoder(flow_sd, xs, c, streaming)
        assert (h[0, :, ::8] - torch.from_numpy(gd[f'h_T{T}_{tag}'])).abs().max() < 2e-5


def test_llm_greedy_ids(golden):
    gd = golden('llm_greedy.npz')
    sd = synth.make_llm(layers=24)
    inp = synth.synthetic_inputs(text_len=int(gd['text_len']), prompt_len=int(gd['prompt_len']),
                                 prompt_text_len=int(gd['prompt_text_len']))
    e0 = torch.zeros(1, 0, dtype=torch.int32)
    for tag, ptxt, ptok in (('zero_shot', inp['prompt_text'], inp['prompt_token']), ('cross_lingual', e0, e0)):
        n = 24      # a prefix keeps the CPU suite short; the GPU parity test runs all 120
        ids, logps = OL.inference(sd, inp['text'], ptxt, ptok, return_logp=True, force_len=None, max_ratio=n / 6)
        assert ids == gd['ids_' + tag][:n].tolist()
        assert np.allclose(torch.stack(logps[:3])[:, ::16].numpy(), gd['logp_head_' + tag], atol=2e-4)


def test_sampler_candidates(golden):
    gd = golden('sampler.npz')
    for logp, cand in zip(gd['logp'], gd['candidates']):
        p, idx = OL.nucleus_candidates(torch.from_numpy(logp), 0.8, 25)
        assert idx == [int(c) for c in cand if c >= 0]
        assert len(idx) <= 25 and (float(p[:-1].sum()) < 0.8 or len(idx) == 1)


def test_sampler_decisions_vs_reference(golden):
    """oracle.llm.sampling_ids against the decisions of the reference's own `TransformerLM.sampling_ids` + `ras_sampling`
    (llm/llm.py:235-250, utils/common.py:111-139) under a committed table of uniforms (tests/golden/make_golden.py gen_sampler_ras: only
    `Tensor.multinomial` is replaced, by an inverse-CDF draw from the table): no repetition, the repetition rule's full-vocabulary re-draw,
    EOS re-draws while ignore_eos, the RuntimeError after 100 re-draws (top = -1), ties."""
    gd = golden('sampler_ras.npz')
    n = len(gd['top'])
    assert n >= 64 and set(gd['kind'].tolist()) == {0, 1, 2, 3, 4}
    fired = errors = redraws = 0
    for i in range(n):
        u = gd['uniforms'][i]
        window = gd['window'][i][:int(gd['window_len'][i])].tolist()
        trials = []

        def uni(step, trial):
            trials.append(trial)
            return float(u[trial, 0]), float(u[trial, 1])
        try:
            top = OL.sampling_ids(torch.from_numpy(gd['logp'][i]), window, bool(gd['ignore_eos'][i]), 'ras', uni, 0)
        except RuntimeError:
            top = -1
        assert top == int(gd['top'][i]), f'case {i} (kind {int(gd["kind"][i])}): oracle {top}, reference {int(gd["top"][i])}'
        assert len(trials) == int(gd['trials'][i])
        fired += int(gd['draws'][i]) > int(gd['trials'][i])
        errors += top == -1
        redraws += int(gd['trials'][i]) > 1
    assert fired >= 8 and errors >= 8 and redraws >= 12          # the fixture exercises every branch


def test_ras_repetition_and_eos_guard():
    logp = torch.full((6564,), -20.0)
    logp[5] = 0.0
    logp = logp.log_softmax(0)
    # nucleus picks 5; 5 appears in the window -> falls back to full-vocab draw with u_random
    assert OL.ras_ids(logp, [1, 2, 3], (0.1, 0.999999999)) == 5
    assert OL.ras_ids(logp, [5, 1, 2], (0.1, 0.999999999)) == 6563      # window hit -> full-vocab draw at u ~ 1
    # EOS re-draw guard: EOS certain while ignore_eos -> RuntimeError after 100 trials (llm/llm.py:242-250)
    logp = torch.full((6564,), -50.0)
    logp[OL.SPEECH_TOKEN_SIZE] = 0.0
    with pytest.raises(RuntimeError):
        OL.sampling_ids(logp.log_softmax(0), [], True, 'ras', lambda s, t: (0.5, 0.5), 0)


def test_llm_bistream_ids(golden):
    """oracle.llm.inference_bistream vs the reference's Qwen2LM.inference_bistream (llm.py:721-834) run under the cache view of
    oracle/ref_harness.py: emitted ids and the out_tokens list (fill / EOS entries included).  One of the four stored cases keeps
    the CPU suite short; the GPU parity test consumes all four."""
    from cv2amd import weights as W
    gd = golden('llm_bistream.npz')
    sd = W.round_llm_sd(synth.make_llm(layers=24))
    b = sd['llm_decoder.bias'].clone()
    b[6563] += float(gd['fill_bias'])
    b[6561] += float(gd['eos_bias'])
    b[6562] = -30.0
    sd['llm_decoder.bias'] = b
    seed = 3
    inp = synth.synthetic_inputs(seed=seed, text_len=int(gd['text_len']), prompt_len=int(gd['prompt_len']), prompt_text_len=int(gd['prompt_text_len']))
    cuts = gd['cuts'].tolist()
    chunks = [inp['text'][:, a:b2] for a, b2 in zip(cuts[:-1], cuts[1:])]
    ids, outs = OL.inference_bistream(sd, chunks, inp['prompt_text'], inp['prompt_token'])
    assert ids == gd[f'ids_prompt_{seed}'].tolist() and outs == gd[f'out_tokens_prompt_{seed}'].tolist()
    assert outs.count(OL.FILL_TOKEN) == 3 and outs[-1] == OL.SPEECH_TOKEN_SIZE


def test_speech_feature_oracles_are_self_consistent():
    """oracle.frontend.whisper_log_mel / kaldi_fbank restate third-party algorithms (openai-whisper, torchaudio: both absent, PARITY-UNPINNED
    against the packages).  What can be pinned here: their torch.stft / torch.fft forms (the packages' own calls) agree with the DFT taken by
    its definition in float64 (framing, window, sign, padding conventions), shapes follow the packages' frame rules, the kaldi banks are
    triangles that cover 20 Hz .. Nyquist, and the product's bank table is the same fp32 table."""
    from oracle import frontend as OFE
    from cv2amd import prompt as P
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 16000 * 2 + 33, generator=g) * 0.1
    a, b = OFE.whisper_log_mel(x), OFE.whisper_log_mel(x, exact_dft=True)
    assert a.shape == b.shape == (1, 128, x.shape[1] // 160) and (a - b).abs().max().item() < 2e-5
    assert a.max().item() - a.min().item() <= 2.0 + 1e-6                    # the max - 8 clamp, scaled by 1 / 4
    k, kd = OFE.kaldi_fbank(x), OFE.kaldi_fbank(x, exact_dft=True)
    assert k.shape == kd.shape == (1 + (x.shape[1] - 400) // 160, 80) and (k - kd).abs().max().item() < 1e-3
    banks = torch.nn.functional.pad(OFE.kaldi_mel_banks(), (0, 1)).numpy()
    assert banks.shape == (80, 257) and (banks >= 0).all() and (banks.max(1) > 0.4).all() and banks[:, 0].max() == 0
    peaks = banks.argmax(1)
    assert (np.diff(peaks) >= 0).all() and peaks[0] >= 1 and peaks[-1] <= 255
    assert np.array_equal(banks, P._kaldi_mel_banks())
