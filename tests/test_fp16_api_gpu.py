"""GPU tests of fp16=True through the drop-in API (CosyVoice2 -> CosyVoice2Model -> FlowEngine(operands='fp16')).  Run with -m gpu on an MI355X.

Three models from the same 2-layer LLM, flow and HiFT state dicts, greedy sampling: fp16 not passed, fp16=False, fp16=True.  The flag must
reach the flow (its mel changes and moves closer to the fp32 oracle) and nothing else (the LLM's ids and the waveform lengths stay the same)."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

TEXT_IDS = {'bonjour': [11, 22, 33, 44, 55, 66, 77, 88], 'guten tag': [9, 8, 7, 6, 5, 4, 3, 2, 1, 10, 20, 30], 'salut': [5, 6, 7, 8, 9, 10],
            'merci': [40, 41, 42, 43, 44, 45, 46, 47, 48, 49]}


@pytest.fixture(scope='module')
def sds():
    from cv2amd import synth
    return synth.make_llm(layers=2), synth.make_flow(), synth.make_hift()


@pytest.fixture(scope='module')
def spk():
    from cv2amd import synth
    inp = synth.synthetic_inputs(prompt_len=37, prompt_text_len=4)
    return {'prompt_text': inp['prompt_text'], 'prompt_text_len': torch.tensor([4]), 'llm_prompt_speech_token': inp['prompt_token'],
            'llm_prompt_speech_token_len': torch.tensor([37]), 'flow_prompt_speech_token': inp['prompt_token'],
            'flow_prompt_speech_token_len': torch.tensor([37]), 'prompt_speech_feat': inp['prompt_feat'],
            'prompt_speech_feat_len': torch.tensor([74]), 'llm_embedding': inp['embedding'], 'flow_embedding': inp['embedding']}


def _model(sds, spk, **kw):
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.frontend import PrecomputedFrontEnd
    fe = PrecomputedFrontEnd(lambda t: TEXT_IDS.get(t.rstrip('.'), [1, 2, 3]), {'fr': spk})
    m = CosyVoice2('unused', final=True, frontend=fe, state_dicts=sds, **kw)
    m.model.sampling_mode = 0            # harness-defined greedy: deterministic tokens
    calls = m.calls = []                 # (finalize, speech tokens) of every flow call: the LLM's ids as the flow receives them
    flow = m.model.flow
    batch0, chunk0 = flow.inference_batch, flow.inference_chunk_batch

    def batch(utts, streaming=False, finalize=True):
        calls.extend((finalize, tuple(u['token'].reshape(-1).tolist())) for u in utts)
        return batch0(utts, streaming=streaming, finalize=finalize)

    def chunk(utts, caches, finalize):
        calls.extend((finalize, tuple(u['token'].reshape(-1).tolist())) for u in utts)
        return chunk0(utts, caches, finalize)
    flow.inference_batch, flow.inference_chunk_batch = batch, chunk
    return m


@pytest.fixture(scope='module')
def models(sds, spk):
    assert torch.cuda.is_available(), 'needs a GPU'
    return {'default': _model(sds, spk), 'bf16': _model(sds, spk, fp16=False), 'fp16': _model(sds, spk, fp16=True)}


def _wave_lengths(m, stream, texts):
    m.calls.clear()
    out = {}

    def one(t):
        out[t] = [o['tts_speech'].shape[1] for o in m.inference_zero_shot(t, 'salut', None, zero_shot_spk_id='fr', stream=stream)]
    th = [threading.Thread(target=one, args=(t,)) for t in texts]
    for x in th:
        x.start()
    for x in th:
        x.join()
    return out, sorted(tok for fin, tok in m.calls if fin)


def _mel(m, spk, tok):
    u = dict(token=torch.tensor(tok, dtype=torch.int32).reshape(1, -1), prompt_token=spk['flow_prompt_speech_token'],
             prompt_feat=spk['prompt_speech_feat'], embedding=spk['flow_embedding'])
    return m.model.flow.inference_batch([u])[0].cpu()


def test_fp16_flag_reaches_the_flow_engine(models):
    assert models['default'].model.flow.operands == 'bf16' and models['bf16'].model.flow.operands == 'bf16'
    assert models['fp16'].model.flow.operands == 'fp16' and models['fp16'].model.fp16 is True


@pytest.mark.parametrize('mode', ['non_stream', 'stream', 'four_concurrent'])
def test_fp16_changes_the_flow_and_nothing_else(models, sds, spk, mode):
    from oracle import flow as OF
    texts = ['bonjour', 'guten tag', 'salut', 'merci'] if mode == 'four_concurrent' else ['bonjour']
    stream = mode == 'stream'
    got = {k: _wave_lengths(models[k], stream, texts) for k in ('bf16', 'fp16', 'default')}
    (len_b, ids_b), (len_h, ids_h), (len_d, ids_d) = got['bf16'], got['fp16'], got['default']
    assert ids_b and ids_b == ids_h == ids_d, 'the LLM ids differ between the models (fp16 must leave the LLM alone)'
    assert len_b == len_h == len_d, (len_b, len_h)
    fsd = sds[1]
    for tok in ids_b[:2]:
        mb, mh, md = (_mel(models[k], spk, tok) for k in ('bf16', 'fp16', 'default'))
        assert torch.equal(mb, md), 'fp16=False is not the default path bit for bit'
        assert not torch.equal(mb, mh), 'fp16=True left the flow mel unchanged'
        ref = OF.inference(fsd, torch.tensor(tok, dtype=torch.int32).reshape(1, -1), spk['flow_prompt_speech_token'], spk['prompt_speech_feat'],
                           spk['flow_embedding'], False, True)
        eb, eh = (mb - ref).abs().max().item(), (mh - ref).abs().max().item()
        assert eh < eb, f'fp16 mel is not closer to the fp32 oracle than the bf16 one ({eh:.3e} vs {eb:.3e})'
