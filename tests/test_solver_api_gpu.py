"""Per-call flow solver settings through the scheduler and the public surface: synthetic weights (2-layer LLM, full-size
flow and HiFT), short texts.  Calls carry a seed (cv2amd.sampling) so that their speech tokens and vocoder noise are functions of the call
alone and two runs can be compared.  Run with -m gpu on an MI355X."""
import pytest
import torch

from test_sampling_api_gpu import Rig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rig():
    return Rig()


def _settings():
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    return Sampling, Solver


def test_non_streaming_call_with_its_own_steps(rig):
    """solver(steps=4) changes the audio, and is token2wav run directly under that setting"""
    from cosyvoice.cli.cosyvoice import CosyVoice2
    Sampling, Solver = _settings()
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling, cv.model = None, False, 24000, None, rig.mdl
    view = cv.solver(steps=4).sampler(seed=5)
    assert view.flow_solver == Solver(steps=4) and cv.flow_solver is None
    (base,), toks0 = rig.call(0, stream=False, sampling=Sampling(seed=5))
    (got,), toks = rig.call(0, stream=False, sampling=view.sampling, solver=view.flow_solver)
    assert toks == toks0 and got.shape == base.shape                # the LLM is not touched by the flow's setting
    assert (got - base).abs().max().item() > 1e-3, 'steps=4 left the audio where 10 steps put it'
    mdl, inp, dev = rig.mdl, rig.inps[0], rig.mdl.device
    uid = 'direct-token2wav'
    mdl.hift_cache_dict[uid], mdl.samp_dict[uid], mdl.solver_dict[uid] = None, [Sampling(seed=5), 0], Solver(steps=4)
    try:
        with mdl.run_lock:
            ref = mdl.token2wav(torch.tensor(toks, dtype=torch.int32).unsqueeze(0), inp['prompt_token'].to(dev), inp['prompt_feat'].to(dev),
                                inp['embedding'].to(dev), 0, uid, finalize=True).cpu()
    finally:
        mdl.hift_cache_dict.pop(uid), mdl.samp_dict.pop(uid), mdl.solver_dict.pop(uid)
    assert ref.shape == got.shape
    err = (got - ref).abs().max().item()
    print(f'solver(steps=4) call vs token2wav under the setting: max abs err {err:.3e}')
    assert err < 1e-3
    assert mdl.solver_dict == {} and mdl.samp_dict == {}
    with pytest.raises(ValueError):
        list(mdl.tts(solver=Solver(steps=40), **rig.kw(0)))


def test_concurrent_streams_with_different_settings_match_themselves_alone(rig):
    Sampling, Solver = _settings()
    jobs = [dict(i=0, sampling=Sampling(seed=11), solver=Solver(steps=4)), dict(i=1, sampling=Sampling(seed=12), solver=Solver(steps=6, cfg_rate=1.0))]
    alone = [rig.call(j['i'], sampling=j['sampling'], solver=j['solver']) for j in jobs]
    plain = rig.call(0, sampling=Sampling(seed=11))
    both = rig.together(jobs)
    for k, ((ca, ta), (cb, tb)) in enumerate(zip(alone, both)):
        assert ta == tb and len(ca) == len(cb) == 3
        for c, (x, y) in enumerate(zip(ca, cb)):
            assert x.shape == y.shape
            err = (x - y).abs().max().item()
            print(f'stream {k} chunk {c}: together vs alone max abs err {err:.3e}')
            assert err < 1e-3, f'stream {k} chunk {c}: max abs err {err:.3e}'
    assert max((x - y).abs().max().item() for x, y in zip(alone[0][0], plain[0])) > 1e-3          # the setting reached the stream's flow
    assert rig.mdl.solver_dict == {} and rig.mdl._flow_caches == {}
