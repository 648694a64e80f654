"""GPU tests of the per-call flow solver settings (cv2_flow_inference_ex / cv2_flow_inference_chunk_ex, csrc/flow.hip): Euler steps and
guidance rate of a call against the reference's own output under the same settings (tests/golden/flow_solver.npz), the default path
unchanged, guidance per utterance in one launch, grouping by step count, the stream cache under a step count of its own, and the
residency of the per-step-count time tables.  Run with -m gpu on an MI355X.

Bars: HIP against the fixture follows the rule of test_flow_gpu.py::test_flow_inference_error_is_explained_by_operand_rounding -- max and
mean distance from the reference's output under 1.25 x the distance of the oracle with operands rounded where the HIP path rounds them, at
the same setting from the same fixture (a CPU quantity, cached per setting).  Everything that compares the engine with itself is
torch.equal, except cached chunks against the recompute (the project's 2e-3 bar, measured bit-identical)."""
import ctypes as C

import pytest
import torch
from _bars import bar

import _solver_oracle as SO

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
def eng(dev, flow_sd):
    from cv2amd.flow import FlowEngine
    return FlowEngine(flow_sd, dev, max_utts=4, max_len=512)


def rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-9)


def mrel(a, b):
    return ((a - b).abs().mean() / b.abs().mean()).item()


def S(steps=None, cfg_rate=None):
    from cv2amd.solver import Solver
    return Solver(steps, cfg_rate)


def _e2e(golden):
    from cv2amd import synth
    ge = golden('flow_e2e.npz')
    return torch.from_numpy(ge['token']), synth.synthetic_inputs(prompt_len=int(ge['prompt_len']))


_ROUNDED = {}


def _rounded(flow_sd, tok, inp, tag, steps, cfg, f16=False):
    """the oracle with rounded operands at this setting (computed once per setting)"""
    from oracle import flow as OF
    k = (tag, steps, cfg, f16)
    if k not in _ROUNDED:
        streaming, finalize = {t: (s, f) for t, s, f in SO.TAGS}[tag]
        bf16_r = OF._r
        if f16:                                                        # oracle.flow._r with fp16 in place of bf16 (tests/golden/make_golden_fp16.py)
            OF._r = lambda x: x.clamp(-65504.0, 65504.0).half().float() if OF.ROUND['on'] else x
        try:
            with OF.rounded_operands():
                _ROUNDED[k] = SO.inference(flow_sd, tok, inp['prompt_token'], inp['prompt_feat'], inp['embedding'], streaming, finalize, steps, cfg)
        finally:
            OF._r = bf16_r
    return _ROUNDED[k]


def _explained(name, got, refr, ref32):
    hip_max, hip_mean, rnd_max, rnd_mean = rel(got, ref32), mrel(got, ref32), rel(refr, ref32), mrel(refr, ref32)
    print(f'{name}: HIP vs reference max {hip_max:.3e} mean {hip_mean:.3e}; rounded oracle vs reference max {rnd_max:.3e} mean {rnd_mean:.3e}')
    bar(f'{name}, max (limit = 1.25 x rounded-operand oracle)', hip_max, 1.25 * rnd_max)
    bar(f'{name}, mean (limit = 1.25 x rounded-operand oracle)', hip_mean, 1.25 * rnd_mean)


@pytest.mark.parametrize('tag', [t for t, _, _ in SO.TAGS])
@pytest.mark.parametrize('steps,cfg', SO.SETTINGS)
def test_solver_settings_vs_reference_golden(golden, eng, flow_sd, steps, cfg, tag):
    tok, inp = _e2e(golden)
    streaming, finalize = {t: (s, f) for t, s, f in SO.TAGS}[tag]
    ref32 = torch.from_numpy(golden('flow_solver.npz')[SO.key(tag, steps, cfg)])
    mel, _ = eng.inference(tok, None, inp['prompt_token'], None, inp['prompt_feat'], None, inp['embedding'], streaming, finalize,
                           solver=S(steps, cfg))
    got = mel.cpu()
    assert got.shape == ref32.shape and torch.isfinite(got).all()
    _explained(f'flow solver steps {steps} cfg {cfg:g} {tag}', got, _rounded(flow_sd, tok, inp, tag, steps, cfg), ref32)


def test_solver_setting_on_an_fp16_engine(golden, dev, flow_sd):
    from cv2amd.flow import FlowEngine
    e16 = FlowEngine(flow_sd, dev, max_utts=1, max_len=256, operands='fp16')
    tok, inp = _e2e(golden)
    steps, cfg = 4, 0.7
    ref32 = torch.from_numpy(golden('flow_solver.npz')[SO.key('full', steps, cfg)])
    mel, _ = e16.inference(tok, None, inp['prompt_token'], None, inp['prompt_feat'], None, inp['embedding'], False, True, solver=S(steps, cfg))
    _explained(f'flow solver steps {steps} cfg {cfg:g} full, fp16 operands', mel.cpu(), _rounded(flow_sd, tok, inp, 'full', steps, cfg, f16=True), ref32)


def _trio():
    from cv2amd import synth
    utts = []
    for i, (p, n) in enumerate(((20, 31), (7, 90), (33, 12))):
        inp = synth.synthetic_inputs(seed=50 + i, prompt_len=p)
        g = torch.Generator().manual_seed(i)
        utts.append(dict(token=torch.randint(0, 6561, (1, n), generator=g, dtype=torch.int32), prompt_token=inp['prompt_token'],
                         prompt_feat=inp['prompt_feat'], embedding=inp['embedding']))
    return utts


def _stream_calls(P, N, hop=25, la=3):
    """(n_tokens_given, token_offset, finalize) of the flow calls of one streaming utterance (cli/model.py:351-381)"""
    pad = -(-P // hop) * hop - P
    calls, off = [], 0
    while N - off >= (hop + pad if off == 0 else hop) + la:
        this = hop + pad if off == 0 else hop
        calls.append((off + this + la, off, False))
        off += this
    calls.append((N, off, True))
    return calls


def _stream(seed, P=20, N=80):
    from cv2amd import synth
    inp = synth.synthetic_inputs(seed=seed, prompt_len=P)
    tok = torch.randint(0, 6561, (1, N), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    calls = _stream_calls(P, N)
    assert len(calls) == 3 and [c[2] for c in calls] == [False, False, True]          # three chunk calls
    return dict(inp=inp, tok=tok, calls=calls, P=P, N=N)


def _utt(st, n):
    return dict(token=st['tok'][:, :n], prompt_token=st['inp']['prompt_token'], prompt_feat=st['inp']['prompt_feat'], embedding=st['inp']['embedding'])


def _run_stream(eng, st, solver, with_solver_kw=True):
    kw = dict(solver=solver) if with_solver_kw else {}
    c = eng.new_cache(2 * (st['P'] + st['N']), **kw)
    outs = []
    for n, off, fin in st['calls']:
        (m, first), = eng.inference_chunk_batch([_utt(st, n)], [c], finalize=fin, **kw)
        outs.append(m.clone())
    return outs


def test_default_path_is_unchanged(eng):
    """Solver() and the explicit engine values are the call without `solver`: bit-identical tensors, batch and cached chunks."""
    utts = _trio()
    base = [m.clone() for m in eng.inference_batch(utts)]
    for sv in (S(), S(10, 0.7), [S(), None, S(10, 0.7)]):
        got = eng.inference_batch(utts, solver=sv)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(base, got)), sv
    st = _stream(71)
    base = _run_stream(eng, st, None, with_solver_kw=False)
    for sv in (S(), S(10, 0.7)):
        got = _run_stream(eng, st, sv)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(base, got)), sv
    assert eng.new_cache(128).buf.numel() == eng.new_cache(128, S(10, 0.7)).buf.numel()


@pytest.mark.parametrize('steps', [None, 4])
def test_guidance_rate_per_utterance_in_one_launch(eng, steps):
    utts = _trio()
    svs = [S(steps, 0.0), S(steps, 0.7 if steps else 0.3), S(steps, 1.5)]
    single = [eng.inference_batch([u], solver=sv)[0].clone() for u, sv in zip(utts, svs)]
    batch = eng.inference_batch(utts, solver=svs)
    torch.cuda.synchronize()
    for s, b in zip(single, batch):
        assert s.shape == b.shape and torch.equal(s, b)
    assert not torch.equal(single[0], eng.inference_batch([utts[0]], solver=S(steps, 1.5))[0])       # the rate reaches the update


def test_mixed_step_counts_are_refused_by_the_entry_point_and_grouped_by_the_engine(eng, dev):
    from cv2amd import lib as L
    from cv2amd.flow import FlowSolver, FlowUtt
    utts = _trio()
    keep, outs = [], []
    arr = (FlowUtt * 3)()
    for i, u in enumerate(utts):
        tok = torch.cat([u['prompt_token'].reshape(-1), u['token'].reshape(-1)]).to(dev, torch.int32).contiguous()
        pf = u['prompt_feat'].reshape(-1, 80).to(dev, torch.float32).contiguous()
        emb = u['embedding'].reshape(-1).to(dev, torch.float32).contiguous()
        out = torch.full((1, 80, 2 * tok.numel() - pf.shape[0]), -77.0, device=dev)
        keep += [tok, pf, emb]
        outs.append(out)
        arr[i] = FlowUtt(tok.data_ptr(), tok.numel(), pf.data_ptr(), pf.shape[0], emb.data_ptr(), out.data_ptr())

    def call(recs):
        sv = (FlowSolver * 3)(*[FlowSolver(n, r) for n, r in recs])
        rc = eng.lib.cv2_flow_inference_ex(eng.handle, arr, sv, 3, 0, 1, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, eng.lib.cv2_last_error().decode()
    rc, msg = call([(4, 0.7), (0, -1.0), (4, 0.7)])                  # utterance 1 resolves to the engine's 10
    assert rc == -1 and 'utterances 0 and 1' in msg and 'step counts' in msg, msg
    for recs in ([(32, 0.7)] * 3, [(4, float('nan'))] * 3, [(4, float('inf'))] * 3):
        rc, msg = call(recs)
        assert rc == -1 and msg, recs
    assert all(bool((o == -77.0).all()) for o in outs)                # no launch followed
    rc, msg = call([(4, 0.7), (4, -1.0), (4, 0.2)])                  # one step count: served
    assert rc == 0, msg
    assert all(bool(torch.isfinite(o).all()) and not bool((o == -77.0).any()) for o in outs)
    # the engine groups: caller's order, bit-identical to the singles
    svs = [S(4, 0.7), S(), S(16, 1.0)]
    single = [eng.inference_batch([u], solver=sv)[0].clone() for u, sv in zip(utts, svs)]
    got = eng.inference_batch(utts, solver=svs)
    torch.cuda.synchronize()
    for s, b in zip(single, got):
        assert s.shape == b.shape and torch.equal(s, b)
    assert torch.equal(outs[0], single[0])
    with pytest.raises(ValueError):
        eng.inference_batch(utts, solver=[S(4)])                       # one setting per utterance
    with pytest.raises(ValueError):
        eng.inference_batch(utts, solver=S(32))


@pytest.mark.parametrize('steps', [4, 16])
def test_cached_chunks_under_a_step_count_equal_the_recompute(eng, steps):
    """steps = 16 > the engine's 10: the cache is laid out and sized by the call's step count"""
    st = _stream(72)
    sv = S(steps, 0.7)
    cache = eng.new_cache(2 * (st['P'] + st['N']), sv)
    assert cache.pair == (steps, eng.pair[1])
    assert cache.buf.numel() == eng.lib.cv2_flow_cache_bytes_ex(eng.handle, cache.frames, steps) != eng.new_cache(2 * (st['P'] + st['N'])).buf.numel()
    for n, off, fin in st['calls']:
        u = _utt(st, n)
        ref = eng.inference_batch([u], streaming=True, finalize=fin, solver=sv)[0][:, :, 2 * off:].clone()
        (got, first), = eng.inference_chunk_batch([u], [cache], finalize=fin, solver=sv)
        torch.cuda.synchronize()
        assert first == 2 * off and got.shape == ref.shape and torch.isfinite(got).all()
        bar(f'flow cached chunk vs recompute, steps {steps}, offset {off}', rel(got.cpu(), ref.cpu()), 2e-3)
    assert cache.n_cached == 2 * (st['P'] + st['N']) and cache.gen == 3


def test_streams_with_different_guidance_rates_share_a_chunk_batch(eng):
    sts, svs = [_stream(73), _stream(74, P=31, N=90)], [S(4, 0.2), S(4, 1.3)]
    alone = [_run_stream(eng, st, sv) for st, sv in zip(sts, svs)]
    caches = [eng.new_cache(2 * (st['P'] + st['N']), sv) for st, sv in zip(sts, svs)]
    for k in range(3):
        fin = sts[0]['calls'][k][2]
        outs = eng.inference_chunk_batch([_utt(st, st['calls'][k][0]) for st in sts], caches, finalize=fin, solver=svs)
        torch.cuda.synchronize()
        for j, (m, _first) in enumerate(outs):
            assert m.shape == alone[j][k].shape
            bar(f'flow cached chunks of 2 streams with their own cfg_rate, stream {j} call {k}', rel(m.cpu(), alone[j][k].cpu()), 2e-3)
    assert not torch.equal(alone[0][0], _run_stream(eng, sts[0], svs[1])[0])


def test_stream_from_a_prompt_cache_of_the_same_pair_and_refusal_of_another(eng):
    from cv2amd import synth
    P, N, sv = 53, 80, S(4, 0.5)                           # 53 - 3 = 50 prompt tokens = 100 frames come from the prompt cache
    inp = synth.synthetic_inputs(seed=93, prompt_len=P)
    tok = torch.randint(0, 6561, (1, N), generator=torch.Generator().manual_seed(8), dtype=torch.int32)
    calls = _stream_calls(P, N)[:-1]
    pc = eng.prompt_cache(inp['prompt_token'], inp['prompt_feat'], inp['embedding'], solver=sv)
    assert pc is not None and pc.n_cached == 100 and pc.gen == 1 and pc.pair == sv.resolve(eng)
    a = eng.new_cache(2 * (P + N), sv)
    b = eng.clone_cache(pc, 2 * (P + N) + 64, sv)
    assert b.n_cached == 100 and b.frames != pc.frames and b.pair == pc.pair
    for n, off, fin in calls:
        u = dict(token=tok[:, :n], prompt_token=inp['prompt_token'], prompt_feat=inp['prompt_feat'], embedding=inp['embedding'])
        (ma, fa), = eng.inference_chunk_batch([u], [a], finalize=False, solver=sv)
        ma = ma.clone()
        (mb, fb), = eng.inference_chunk_batch([u], [b], finalize=False, solver=sv)
        torch.cuda.synchronize()
        assert fa == fb and ma.shape == mb.shape
        bar(f'flow prompt-cache start vs recompute under a solver setting, offset {off}', rel(mb.cpu(), ma.cpu()), 2e-3)
    # a cache used under another pair: refused, and left where it was
    u = dict(token=tok, prompt_token=inp['prompt_token'], prompt_feat=inp['prompt_feat'], embedding=inp['embedding'])
    state = (a.n_cached, a.gen)
    for other in (None, S(4, 0.7), S(5, 0.5), S(cfg_rate=0.5)):
        with pytest.raises(ValueError, match='flow cache'):
            eng.inference_chunk_batch([u], [a], finalize=True, solver=other)
    for other in (S(), S(4, 0.7), S(16, 0.5)):
        with pytest.raises(ValueError, match='flow cache'):
            eng.clone_cache(pc, 512, other)
    assert (a.n_cached, a.gen) == state
    with pytest.raises(ValueError, match='one step count'):
        eng.inference_chunk_batch([u, u], [a, eng.new_cache(64, S(6, 0.5))], finalize=True, solver=[sv, S(6, 0.5)])


def test_time_tables_stay_resident_and_leave_the_estimator_seam_alone(eng, dev):
    T = 50
    g = torch.Generator().manual_seed(9)
    x, mu, cond = (torch.randn(2, 80, T, generator=g).to(dev) for _ in range(3))
    spks, t = torch.randn(2, 80, generator=g).to(dev), torch.full((2,), 0.62, device=dev)

    def est():
        return eng.forward_estimator(x.clone().contiguous(), torch.ones(2, 1, T, device=dev), mu, t, spks, cond).clone()
    utts = _trio()[:1]
    e0 = est()
    a4 = eng.inference_batch(utts, solver=S(4))[0].clone()
    d0 = eng.inference_batch(utts)[0].clone()
    e1 = est()                                                       # writes slot 31 of the engine's table
    b4 = eng.inference_batch(utts, solver=S(4))[0].clone()
    a31 = eng.inference_batch(utts, solver=S(31))[0].clone()        # the last rows of the extra region
    d1 = eng.inference_batch(utts)[0].clone()
    c4 = eng.inference_batch(utts, solver=S(4))[0].clone()
    e2 = est()
    torch.cuda.synchronize()
    assert torch.equal(a4, b4) and torch.equal(a4, c4) and torch.equal(d0, d1) and torch.equal(e0, e1) and torch.equal(e0, e2)
    assert not torch.equal(a4, d0) and torch.isfinite(a31).all()
