"""GPU tests of the fp16 flow engine (FlowEngine(operands='fp16'), the reference's fp16=True): every matrix-product operand of the flow rounded
to fp16 (nearest even, saturated to +-65504) instead of bf16, fp32 everything else.  Run with -m gpu on an MI355X.

The bars follow the bf16 engine's rules (tests/test_flow_gpu.py, tests/test_heavytail_gpu.py): the HIP path's distance from the fp32 oracle must
be explained by operand rounding alone -- here the oracle in fp16 rounded-operand mode (oracle.flow._r swapped for saturating fp16 rounding,
the same swap tests/golden/make_golden_fp16.py makes) -- and, fp16 keeping 11 significant bits to bf16's 8, the fp16 engine's error must be
at most a quarter of the bf16 engine's on the same inputs (predicted an eighth)."""
import contextlib
import json
import os

import numpy as np
import pytest
from _bars import bar, _OUT as OUT      # (the directory where the bars' record goes)
import torch

pytestmark = pytest.mark.gpu



@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def flow_sd():
    from cv2amd import synth
    return synth.make_flow()


@pytest.fixture(scope='module')
def eng16(dev, flow_sd):
    from cv2amd.flow import FlowEngine
    e = FlowEngine(flow_sd, dev, max_utts=4, max_len=512, operands='fp16')
    assert e.operands == 'fp16'
    return e


@pytest.fixture(scope='module')
def eng(dev, flow_sd):
    from cv2amd.flow import FlowEngine
    return FlowEngine(flow_sd, dev, max_utts=4, max_len=512)


def rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-9)


def mrel(a, b):
    return ((a - b).abs().mean() / b.abs().mean()).item()


def _record(name, **vals):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'flow_fp16_errors.jsonl'), 'a') as f:
        f.write(json.dumps(dict(test=name, **vals)) + '\n')


@contextlib.contextmanager
def f16_operands():
    """The oracle with every matrix-product operand rounded to fp16 (saturating) where the HIP path rounds it."""
    from oracle import flow as OF
    r0 = OF._r
    OF._r = lambda x: x.clamp(-65504.0, 65504.0).half().float() if OF.ROUND['on'] else x
    try:
        with OF.rounded_operands():
            yield
    finally:
        OF._r = r0


def _check_explained(name, y16, y16b, ref32, refr, max_ratio=1.25):
    """fp16 HIP vs fp32 within max_ratio (max) / 1.25 (mean) of fp16 operand rounding alone; fp16 max <= 0.25 x the bf16 engine's."""
    hm, hn, rm, rn, bm = rel(y16, ref32), mrel(y16, ref32), rel(refr, ref32), mrel(refr, ref32), rel(y16b, ref32)
    _record(name, hip_f16_vs_fp32_max=hm, hip_f16_vs_fp32_mean=hn, rounded_f16_vs_fp32_max=rm, rounded_f16_vs_fp32_mean=rn,
            hip_bf16_vs_fp32_max=bm, hip_bf16_vs_fp32_mean=mrel(y16b, ref32), f16_over_bf16_max=hm / max(bm, 1e-30))
    assert torch.isfinite(y16).all()
    bar(f'fp16 {name}: HIP-vs-fp32 max / fp16-rounded-oracle max', hm / rm, max_ratio)
    bar(f'fp16 {name}: HIP-vs-fp32 mean / fp16-rounded-oracle mean', hn / rn, 1.25)
    bar(f'fp16 {name}: fp16 engine max error / bf16 engine max error', hm / bm, 0.25)


def test_gemm_f16_matches_fp64(dev):
    from cv2amd import lib as L, weights as W
    from cv2amd import flow as F
    lib = L.lib()
    F._bind(lib)
    g = torch.Generator().manual_seed(0)
    # the nine shapes of test_gemm_bf16_matches_fp64: row-panel kernel, 64x128 / 128x128 / 64x256 tiles, the large-grid configurations
    for m, n, k in ((128, 128, 64), (256, 256, 256), (384, 1536, 256), (128, 256, 768), (256, 1024, 1024), (128, 512, 2560),
                    (16384, 256, 512), (6400, 1024, 256), (3072, 1536, 256)):
        a = torch.randn(m, k, generator=g)
        w = torch.randn(n, k, generator=g) / k ** 0.5
        b = torch.randn(n, generator=g)
        ah = a.half().to(dev)
        wp = W.pack_f16(w.to(dev))
        out = torch.full((m, n), float('nan'), device=dev)
        L.check(lib.cv2_gemm_f16(ah.data_ptr(), k, wp.data_ptr(), b.to(dev).data_ptr(), out.data_ptr(), n, m, n, k, L.stream_ptr()))
        torch.cuda.synchronize()
        ref = ah.cpu().double() @ W.f16_round(w).double().T + b.double()
        err = (out.cpu().double() - ref).abs().max().item()
        bar(f'cv2_gemm_f16 vs fp64 m={m} n={n} k={k} (abs err / (1 + max|ref|))', err / (1 + ref.abs().max().item()), 2e-5)


def _est_inputs(seed, T):
    g = torch.Generator().manual_seed(seed)
    x, mu, cond = (torch.randn(2, 80, T, generator=g) for _ in range(3))
    spks = torch.randn(2, 80, generator=g)
    return x, mu, cond, spks


def _run_est(e, dev, x, mu, cond, spks, t, streaming):
    T = x.shape[2]
    return e.forward_estimator(x.to(dev).contiguous(), torch.ones(2, 1, T, device=dev), mu.to(dev), t.to(dev), spks.to(dev), cond.to(dev),
                               streaming).cpu()


@pytest.mark.parametrize('streaming', [False, True])
def test_estimator_f16_error_is_explained_by_fp16_operand_rounding(eng16, eng, dev, flow_sd, streaming):
    from oracle import flow as OF
    T = 150
    x, mu, cond, spks = _est_inputs(9, T)
    t = torch.full((2,), 0.62)
    y16 = _run_est(eng16, dev, x, mu, cond, spks, t, streaming)
    yb = _run_est(eng, dev, x, mu, cond, spks, t, streaming)
    ref32 = OF.estimator(flow_sd, x, torch.ones(2, 1, T), mu, t, spks, cond, streaming)
    with f16_operands():
        refr = OF.estimator(flow_sd, x, torch.ones(2, 1, T), mu, t, spks, cond, streaming)
    _check_explained('estimator_T150_' + ('chunk' if streaming else 'full'), y16, yb, ref32, refr)


@pytest.mark.parametrize('tag,streaming,finalize', [('full', False, True), ('stream', True, True), ('stream_nonfinal', True, False)])
def test_flow_f16_inference_vs_reference_golden(golden, eng16, eng, flow_sd, tag, streaming, finalize):
    from cv2amd import synth
    from oracle import flow as OF
    gd = golden('flow_e2e.npz')
    inp = synth.synthetic_inputs(prompt_len=int(gd['prompt_len']))
    tok = torch.from_numpy(gd['token'])
    args = (tok, None, inp['prompt_token'], None, inp['prompt_feat'], None, inp['embedding'], streaming, finalize)
    y16, yb = eng16.inference(*args)[0].cpu(), eng.inference(*args)[0].cpu()
    ref32 = torch.from_numpy(gd['mel_' + tag])
    with f16_operands():
        refr = OF.inference(flow_sd, tok, inp['prompt_token'], inp['prompt_feat'], inp['embedding'], streaming, finalize)
    assert y16.shape == ref32.shape == refr.shape
    _check_explained('flow_e2e_' + tag, y16, yb, ref32, refr)


@pytest.fixture(scope='module')
def flows_1010(dev):
    from cv2amd import synth
    from cv2amd.flow import FlowEngine
    sd = synth.make_flow()
    return FlowEngine(sd, dev, max_utts=1, max_len=1100, operands='fp16'), FlowEngine(sd, dev, max_utts=1, max_len=1100)


def _fullsize_mels(golden, flows_1010):
    from cv2amd import synth
    gd = golden('fullsize.npz')
    inp = synth.synthetic_inputs(prompt_len=int(gd['prompt_len']))
    args = (torch.from_numpy(gd['token']), None, inp['prompt_token'], None, inp['prompt_feat'], None, inp['embedding'], False, True)
    return [f.inference(*args)[0] for f in flows_1010]


def test_flow_f16_config1_shape_vs_reference_golden(golden, flows_1010):
    """configs[1] (P = 255, 250 tokens, T = 1010): the reference's own mel; fp16-rounded oracle = tests/golden/chain_rounded_f16.npz."""
    y16, yb = (m.cpu() for m in _fullsize_mels(golden, flows_1010))
    ref32 = torch.from_numpy(golden('fullsize.npz')['mel']).unsqueeze(0)
    refr = torch.from_numpy(golden('chain_rounded_f16.npz')['mel_rounded']).unsqueeze(0)
    assert y16.shape == ref32.shape == refr.shape == (1, 80, 500)
    _check_explained('flow_T1010', y16, yb, ref32, refr)


@pytest.mark.parametrize('streaming', [False, True])
def test_heavy_tailed_flow_f16_error_is_explained_by_fp16_operand_rounding(dev, streaming):
    from cv2amd import synth
    from cv2amd.flow import FlowEngine
    from oracle import flow as OF
    sd = synth.heavy_tail_flow(synth.make_flow())
    e = FlowEngine(sd, dev, max_utts=2, max_len=256, operands='fp16')
    T = 150
    x, mu, cond, spks = _est_inputs(19, T)
    t = torch.full((2,), 0.41)
    y = _run_est(e, dev, x, mu, cond, spks, t, streaming)
    ref32 = OF.estimator(sd, x, torch.ones(2, 1, T), mu, t, spks, cond, streaming)
    with f16_operands():
        refr = OF.estimator(sd, x, torch.ones(2, 1, T), mu, t, spks, cond, streaming)
    hm, hn, rm, rn = rel(y, ref32), mrel(y, ref32), rel(refr, ref32), mrel(refr, ref32)
    _record('flow_heavy_estimator_' + ('chunk' if streaming else 'full'), hip_f16_vs_fp32_max=hm, hip_f16_vs_fp32_mean=hn,
            rounded_f16_vs_fp32_max=rm, rounded_f16_vs_fp32_mean=rn, out_range=float(ref32.abs().max()))
    assert torch.isfinite(y).all()
    bar(f'fp16 heavy-tail flow ({"chunk" if streaming else "full"}): HIP-vs-fp32 max / fp16-rounded max', hm / rm, 1.3)
    bar(f'fp16 heavy-tail flow ({"chunk" if streaming else "full"}): HIP-vs-fp32 mean / fp16-rounded mean', hn / rn, 1.25)


def test_estimator_f16_saturates_instead_of_overflowing(dev, flow_sd):
    """One feed-forward input projection scaled up so that its GELU output -- the operand of the next GEMM -- exceeds the fp16 range in the
    fp32 oracle: the fp16 engine saturates it to 65504 (finite output) where an unsaturated conversion would give inf and NaN downstream."""
    from cv2amd.flow import FlowEngine
    from oracle import flow as OF
    key = 'decoder.estimator.mid_blocks.5.1.2.ff.net.0.proj.weight'
    sd = dict(flow_sd)
    sd[key] = flow_sd[key] * 3e4
    T = 150
    x, mu, cond, spks = _est_inputs(29, T)
    t = torch.full((2,), 0.5)
    seen = {'max': 0.0}
    r0 = OF._r

    def record(v):                                   # the fp32 oracle, recording the largest matrix-product operand it forms
        seen['max'] = max(seen['max'], float(v.abs().max()))
        return v
    OF._r = lambda v: record(v) if OF.ROUND['on'] else v
    try:
        with OF.rounded_operands():
            ref32 = OF.estimator(sd, x, torch.ones(2, 1, T), mu, t, spks, cond, False)
    finally:
        OF._r = r0
    assert seen['max'] > 65504.0, f'the scaled projection does not leave the fp16 range ({seen["max"]:.4g})'
    e = FlowEngine(sd, dev, max_utts=1, max_len=256, operands='fp16')
    y = _run_est(e, dev, x, mu, cond, spks, t, False)
    assert torch.isfinite(y).all(), 'fp16 estimator output holds inf / NaN'
    with f16_operands():
        refr = OF.estimator(sd, x, torch.ones(2, 1, T), mu, t, spks, cond, False)
    _record('saturation', largest_fp32_operand=seen['max'], hip_vs_saturating_oracle_max=rel(y, refr), hip_vs_saturating_oracle_mean=mrel(y, refr),
            hip_vs_fp32_max=rel(y, ref32))


def _utt(seed, p, n):
    from cv2amd import synth
    inp = synth.synthetic_inputs(seed=seed, prompt_len=p)
    g = torch.Generator().manual_seed(seed)
    return dict(token=torch.randint(0, 6561, (1, n), generator=g, dtype=torch.int32), prompt_token=inp['prompt_token'],
                prompt_feat=inp['prompt_feat'], embedding=inp['embedding'])


def test_f16_ragged_batch_equals_single(eng16):
    utts = [_utt(50 + i, p, n) for i, (p, n) in enumerate(((20, 31), (7, 90), (33, 12)))]
    single = [eng16.inference_batch([u])[0].clone() for u in utts]
    batch = eng16.inference_batch(utts)
    torch.cuda.synchronize()
    for s, b in zip(single, batch):
        assert s.shape == b.shape and torch.equal(s, b)


def _stream_calls(P, N, hop=25, la=3):
    """Token counts of the flow calls of one streaming utterance (cli/model.py:351-381), as tests/test_flow_gpu.py walks them."""
    pad = -(-P // hop) * hop - P
    calls, off = [], 0
    while True:
        this = hop + pad if off == 0 else hop
        if N - off >= this + la:
            calls.append((off + this + la, off, False))
            off += this
        else:
            break
    calls.append((N, off, True))
    return calls


def test_f16_cached_chunks_equal_the_recompute_of_the_whole_prefix(eng16):
    """cv2_flow_inference_chunk on an fp16 engine: the stream cache holds fp16 keys / values and conv tails."""
    from cv2amd import synth
    P, N = 37, 150
    inp = synth.synthetic_inputs(seed=91, prompt_len=P)
    tok = torch.randint(0, 6561, (1, N), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    cache = eng16.new_cache(2 * (P + N))
    for n, off, fin in _stream_calls(P, N):
        u = dict(token=tok[:, :n], prompt_token=inp['prompt_token'], prompt_feat=inp['prompt_feat'], embedding=inp['embedding'])
        ref = eng16.inference_batch([u], streaming=True, finalize=fin)[0][:, :, 2 * off:].clone()
        (got, first), = eng16.inference_chunk_batch([u], [cache], finalize=fin)
        torch.cuda.synchronize()
        assert first == 2 * off and got.shape == ref.shape and torch.isfinite(got).all()
        bar(f'fp16 flow cached chunk vs recompute, offset {off}', rel(got.cpu(), ref.cpu()), 2e-3)     # (bf16: measured 0.0)


def test_f16_batch_of_32_agrees_with_single(dev, flow_sd):
    """32 utterances select the batch kernels (k_tail_rows2 with the chained QKV projection, k_attn_est_dma<.., 2>) in their fp16 forms."""
    from cv2amd.flow import FlowEngine
    big = FlowEngine(flow_sd, dev, max_utts=32, max_len=2 * (310 + 300) + 8, operands='fp16')
    g = torch.Generator().manual_seed(7)
    utts = [_utt(8000 + b, 255 if b % 2 == 0 else 310, int(torch.randint(150, 301, (1,), generator=g))) for b in range(32)]
    batch = [m.clone() for m in big.inference_batch(utts)]
    for i in (0, 17, 31):
        single = big.inference_batch([utts[i]])[0]
        torch.cuda.synchronize()
        assert single.shape == batch[i].shape and torch.isfinite(batch[i]).all()
        bar(f'fp16 flow batch-of-32 vs single, utterance {i}', rel(batch[i].cpu(), single.cpu()), 1e-2)


def test_chain_f16_tokens_to_waveform_vs_reference_chain(golden, flows_1010, dev):
    """test_chain_tokens_to_waveform_vs_reference_chain (tests/test_fullsize_gpu.py) with the fp16 flow engine: same tokens, same noise, same
    oracle HiFT for the reference chain.  LSD <= 1.25 x what fp16 operand rounding alone gives in the oracle; the chain's mel at most a quarter as
    far from the reference's as the bf16 engine's; the f0 bars of the bf16 test."""
    import _metrics as M
    from cv2amd import synth
    from cv2amd.hift import HiftEngine
    from oracle import hift as OH
    gd = golden('fullsize.npz')
    T = 500
    g = torch.Generator().manual_seed(int(gd['noise_seed']))
    ri, nz = torch.rand(1, 9, generator=g), torch.randn(1, 480 * T, 9, generator=g)
    hsd = synth.make_hift()
    mel16, melb = _fullsize_mels(golden, flows_1010)
    heng = HiftEngine(hsd, dev, max_frames=512)
    wav16 = heng.inference(mel16, None, noise=nz)[0].cpu()[0]
    f0_16 = heng.debug_f0(T).cpu()
    wavb = heng.inference(melb, None, noise=nz)[0].cpu()[0]
    torch.cuda.synchronize()
    mel_ref = torch.from_numpy(gd['mel']).unsqueeze(0)
    wav_ref = OH.inference(hsd, mel_ref, torch.zeros(1, 1, 0), ri, nz)[0][0]
    f0_ref = OH.f0_predictor(hsd, mel_ref).reshape(-1)
    mel_rnd = torch.from_numpy(golden('chain_rounded_f16.npz')['mel_rounded']).unsqueeze(0)
    wav_rnd = OH.inference(hsd, mel_rnd, torch.zeros(1, 1, 0), ri, nz)[0][0]
    lsd16, lsdb, lsd_rnd = M.lsd_mel_db(wav_ref, wav16), M.lsd_mel_db(wav_ref, wavb), M.lsd_mel_db(wav_ref, wav_rnd)
    pm = M.pitch_metrics(f0_ref.numpy(), f0_16.numpy())
    rec = {'lsd_mel_db_fp16': lsd16, 'lsd_mel_db_bf16': lsdb, 'lsd_mel_db_fp16_operand_rounding_in_the_oracle': lsd_rnd, 'pitch_fp16': pm,
           'mel_rel_max_fp16': rel(mel16.cpu(), mel_ref), 'mel_rel_max_bf16': rel(melb.cpu(), mel_ref),
           'sample_corr_fp16': float(np.corrcoef(wav16.numpy(), wav_ref.numpy())[0, 1])}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'chain_tolerance_fp16.json'), 'w') as f:
        json.dump(rec, f)
    assert pm['voiced_pairs'] >= 400, pm
    bar('fp16 chain: LSD relative to fp16 operand rounding alone in the oracle', lsd16 / max(lsd_rnd, 1e-9), 1.25)
    # The LSD does NOT fall with the mel error (first run: fp16 3.20 dB, bf16 engine 3.15, the fp16-rounded oracle 3.20, the bf16-rounded one 3.40,
    # while the fp16 mel is 8x closer to the reference's): any mel perturbation of this size moves the sine source's integrated phase, the two
    # waveforms decorrelate alike (sample correlation 0.75 in both chains), and the log-mel distance saturates near 3.2 dB.  So the gain of the
    # fp16 flow is held on the chain's mel, and on the f0 track below; the LSD against the bf16 engine's is recorded, not barred.
    bar('fp16 chain: mel distance from the reference / the bf16 engine\'s', rel(mel16.cpu(), mel_ref) / rel(melb.cpu(), mel_ref), 0.25)
    bar('fp16 chain: gross pitch error of the f0 tracks, %', pm['gpe'], 0.5)
    bar('fp16 chain: f0 RMSE on voiced frames, Hz', pm['f0_rmse_hz'], 0.5)
    bar('fp16 chain: 1 - f0 correlation', 1.0 - pm['f0_corr'], 1e-4)
    bar('fp16 chain: voiced / unvoiced mismatch, %', pm['vuv'], 0.5)
