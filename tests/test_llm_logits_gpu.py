"""The LLM decode step's LOGITS, in every form the engine takes, against the fp64 oracle.  Run with -m gpu on an MI355X.

Every other decode test compares token ids: an argmax test, blind to an error below a top-1 margin (~0.7 on logits of ~13).  Here
each case prefills, then steps ONE step at a time through the C ABI and reads `cv2_llm_io.logits` after every step.  The oracle is
teacher-forced with the ids the DEVICE emitted (oracle.llm.logit_trace), so a comparison never depends on ids agreeing.  Three
traces per row: fp64 (the reference), fp32 with the decode path's operand rounding (oracle.llm.split_operands: the model of what
the HIP path is allowed to cost) and plain fp32.  Distances are max and rms over the vocabulary of |delta logit|, relative to that
step's max |logit|; per case the maximum over all rows and decode steps.

The bars: HIP max <= 1.5 x model max and HIP rms <= 1.5 x model rms.  1.5: two independent realisations of the same rounding
(the model with its K sums in one piece, in four chunks, in fp64) differ by up to 1.26x / 1.32x on the CPU; the flow's equivalent
bars are 1.25 - 1.3; the HIP path adds fp32 accumulation in an order of its own.  The model fixes the bar, the code under test
never does.  Every ratio goes through _bars.bar (bars.jsonl in its output directory), the raw distances to llm_logit_distances.jsonl beside it.

Which logits row holds what (from csrc/llm.hip, not assumed): cv2_llm_prefill leaves the last prompt row's logits in row
(len - 1) % 32 (the last 32-row pass, :2642); cv2_llm_prefill_batch / cv2_llm_extend_batch in row i of the call's slot list
(k_gather_rows + the head over n rows, :2753-2763); a decode step in row r of the step -- slot r for cv2_llm_decode, slot slots[r]
for cv2_llm_decode_rows (`a.logits += row * ldl`, :962; the launches' head writes its rows in order, :2490)."""
import contextlib
import ctypes as C

import pytest
import torch

from _bars import bar
from _llm_trace import dist, record

pytestmark = pytest.mark.gpu

EOS = 6561
STEPS = 8


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a GPU'
    return torch.device('cuda:0')


class Rig:
    """One checkpoint on one engine plus the oracle's two state dicts (bf16-rounded GEMM weights in fp32 and in fp64)."""
    def __init__(self, sd, dev, **kw):
        from cv2amd import weights as W
        from cv2amd.llm import LLMEngine
        from oracle import llm as OL
        self.sdr = W.round_llm_sd(sd)
        self.sd64 = {k: v for k, v in OL.to_fp64(self.sdr).items() if k != 'llm.model.model.embed_tokens.weight'}    # (unused by a trace)
        self.eng = LLMEngine(sd, dev, **kw)


def _make(layers, dev, heavy=False, **kw):
    from cv2amd import synth
    sd = synth.make_llm(layers=layers)
    return Rig(synth.heavy_tail_llm(sd) if heavy else sd, dev, **kw)


@pytest.fixture(scope='module')
def rig3(dev):
    """3 layers, 32 slots, 1024 positions: 8 attention tiles of 128 keys, the one-launch forms up to 24 rows, the launches to 32"""
    return _make(3, dev, max_seqs=32, max_pos=1024, max_out=64)


@pytest.fixture(scope='module')
def rig24(dev):
    return _make(24, dev, max_seqs=32, max_pos=512, max_out=64)


def _x(eng, seed, length):
    """an lm_input of exactly `length` rows: [sos, 5 text ids, task id, length - 7 prompt speech ids]"""
    from cv2amd import synth
    assert length >= 8
    inp = synth.synthetic_inputs(seed=seed, text_len=5, prompt_len=length - 7, prompt_text_len=0)
    x = eng.build_lm_input(inp['text'], inp['prompt_text'], inp['prompt_token'])
    assert x.shape[0] == length
    return x


def _lengths(n, base=12):
    """a different prompt length for every row (every row its own position and attention-tile fill)"""
    return [base + (7 * r) % 29 + r for r in range(n)]


def _one_launch(eng, n_rows, shared):
    """the form cv2_llm_decode_ex / cv2_llm_decode_rows will take (csrc/llm.hip: `one_launch` in cv2_llm_decode_ex and cv2_llm_decode_rows; CH_ROWS_DEFAULT = 24)"""
    return bool(eng.lib.cv2_llm_one_launch_step(eng.handle)) and not shared and not eng.chain_broken and n_rows <= 24


def _greedy_ok(lg, tok):
    """the id k_sample must draw in greedy forced-length mode: argmax over the ids below EOS, ties -> the lowest id (llm.hip: the masks at the top of k_sample)"""
    return int(lg[:EOS].argmax()) == tok


def _drive(rig, xs, slots, steps, shared, want_one_launch, mode=0, seed=0, feed=None):
    """Prefill `xs` into `slots`, then `steps` single decode steps (rows = slots in list order).  feed = (after_step, blocks): after
    that many steps every slot is given blocks[i] (rows [len_i, hidden]) through cv2_llm_extend_batch at its current position
    instead of its pending token.  Returns per row the stages [(kind, arg)], the device logits [stages, vocab] and the drawn ids."""
    from cv2amd import lib as L
    eng = rig.eng
    n, V = len(slots), eng.vocab
    assert _one_launch(eng, n, shared) == want_one_launch, f'{n} rows, shared={shared}: not the intended step form'
    lockstep = list(slots) == list(range(n))
    total = steps + 1 + (1 if feed else 0)
    eng.park()
    eng.add_requests(list(slots), xs, [(total, total)] * n, mode, seed, True)
    torch.cuda.synchronize()
    logits = [eng.logits[:n, :V].cpu().clone()]
    stages = [[('rows', x.cpu())] for x in xs]                    # what the oracle is fed per stage; ids are filled in afterwards
    for j in range(steps):
        if feed and j == feed[0]:
            st = eng.state.cpu()
            pos0 = [int(st[s, L.ST_POS]) for s in slots]
            assert pos0 == [x.shape[0] + j for x in xs]          # the block goes where the pending token would have gone
            emb = torch.cat(feed[1], 0).to(eng.device).contiguous()
            arr = lambda v: (C.c_int32 * n)(*v)                   # noqa: E731
            L.check(eng.lib.cv2_llm_extend_batch(eng.handle, n, arr(slots), arr([b.shape[0] for b in feed[1]]), arr(pos0), L.ptr(emb),
                                                 L.stream_ptr()))
            torch.cuda.synchronize()
            logits.append(eng.logits[:n, :V].cpu().clone())
            for r in range(n):
                stages[r].append(('rows', feed[1][r].cpu()))
        if lockstep:
            eng.step(n, 1, shared=shared)
        else:
            eng.step_rows(list(slots), 1, shared=shared)
        torch.cuda.synchronize()
        logits.append(eng.logits[:n, :V].cpu().clone())
        for r in range(n):
            stages[r].append(('tok', None))
    st = eng.state.cpu()
    toks = eng.out_tokens.cpu()
    assert not eng.chain_broken, 'a hand-off timed out: the steps were not all taken in the intended form'
    ids = []
    for r, s in enumerate(slots):
        assert int(st[s, L.ST_ERR]) == 0 and int(st[s, L.ST_NOUT]) == total and int(st[s, L.ST_DONE]) == 1
        ids.append(toks[s, :total].tolist())
    eng.park()
    return stages, torch.stack(logits, 1), ids                    # logits [n, stages, V]; ids[r][j] was drawn from stage j's logits


def _oracle(rig, stages, ids):
    """fp64, split-operand and fp32 traces of one row under the device's ids: each [stages, vocab]"""
    from oracle import llm as OL
    out = []
    for sd, split in ((rig.sd64, False), (rig.sdr, True), (rig.sdr, False)):
        t = OL.LogitTrace(sd)
        rows = []
        with OL.split_operands() if split else contextlib.nullcontext():
            for j, (kind, arg) in enumerate(stages):
                # a token stage feeds the id drawn from the stage before it -- unless a block replaced it (then ids[j - 1] is never fed)
                rows.append(t.feed(arg.float()) if kind == 'rows' else t.step(ids[j - 1]))
        out.append(torch.stack(rows))
    return out


def _check(name, rig, xs, slots, steps=STEPS, shared=False, one_launch=True, mode=0, seed=0, feed=None, cap=True):
    stages, logits, ids = _drive(rig, xs, slots, steps, shared, one_launch, mode, seed, feed)
    assert torch.isfinite(logits).all()
    hip, mod, f32 = [], [], []
    for r in range(len(slots)):
        if mode == 0:                                             # k_sample: every greedy id is the argmax of the device's own logits
            for j, t in enumerate(ids[r]):
                assert _greedy_ok(logits[r, j], t), f'{name}: row {r} stage {j}: id {t} is not the argmax of the logits it was drawn from'
        ref, m, f = _oracle(rig, stages[r], ids[r])
        hip.append(torch.stack(dist(logits[r], ref)))             # [2 (max, rms), stages]
        mod.append(torch.stack(dist(m, ref)))
        f32.append(torch.stack(dist(f, ref)))
    hip, mod, f32 = torch.stack(hip), torch.stack(mod), torch.stack(f32)          # [rows, 2, stages]
    dec = slice(1, None)                                          # stage 0 is the prefill (recorded; the bars are the decode steps')
    agg = lambda t: (t[:, 0, dec].max().item(), t[:, 1, dec].max().item())        # noqa: E731
    (hm, hr), (mm, mr), (fm, fr) = agg(hip), agg(mod), agg(f32)
    worst = (hip[:, 0, dec].amax(1) / mod[:, 0, dec].amax(1))
    record(name, rows=len(slots), steps=steps, hip_max=hm, hip_rms=hr, model_max=mm, model_rms=mr, fp32_max=fm, fp32_rms=fr,
           prefill_hip_max=hip[:, 0, 0].max().item(), prefill_model_max=mod[:, 0, 0].max().item(),
           worst_row=int(worst.argmax()), worst_row_ratio=worst.max().item())
    print(f'{name}: HIP {hm:.2e} / {hr:.2e}  model {mm:.2e} / {mr:.2e}  fp32 {fm:.2e} / {fr:.2e}  ratios {hm / mm:.2f} / {hr / mr:.2f}')
    if cap:
        assert mm < 2e-4, f'{name}: the split-operand model itself is {mm:.2e} from fp64'       # (the cap of the CPU test, on this case's ids)
    bar(f'llm logits {name}: HIP max / model max', hm / mm, 1.5, f'(HIP {hm:.3e}, model {mm:.3e}, fp32 {fm:.3e})')
    bar(f'llm logits {name}: HIP rms / model rms', hr / mr, 1.5, f'(HIP {hr:.3e}, model {mr:.3e}, fp32 {fr:.3e})')


# ---- every step form ------------------------------------------------------------------------------------------------------------
# one launch: 1 row k_step, 3 rows k_step<true>, 2 / 5 / 6 / 8 rows k_step_rows<2> (5: a half-empty last pair, 6: three full pairs),
# 9 / 10 / 11 / 13 / 16 / 24 rows k_step_rows<4> (9 and 13: a last chain of 1 row, 10: of 2 -- its second O block has no row and returns
# early --, 11: of 3, 24: full); shared=True: the launches, 17 / 25 / 32 rows: prepared operands
@pytest.mark.parametrize('n', [1, 2, 3, 5, 6, 8, 9, 10, 11, 13, 16, 24])
def test_one_launch_forms(rig3, n):
    eng = rig3.eng
    xs = [_x(eng, 100 * n + r, ln) for r, ln in enumerate(_lengths(n))]
    _check(f'one-launch step, {n} rows', rig3, xs, range(n), shared=False, one_launch=True)


@pytest.mark.parametrize('n', [1, 2, 3, 5, 8, 9, 11, 13, 16, 17, 25, 32])
def test_launch_forms(rig3, n):
    eng = rig3.eng
    xs = [_x(eng, 100 * n + r, ln) for r, ln in enumerate(_lengths(n))]
    _check(f'launches, {n} rows', rig3, xs, range(n), shared=True, one_launch=False)


# ---- tile and split edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('edge', [128, 256, 512])
@pytest.mark.parametrize('n', [1, 2, 9])
def test_context_walks_across_a_tile_edge(rig3, n, edge, shared):
    """Prompts of edge - 4 .. edge - 1 rows: the 8 decode steps walk every row's context (cached keys + the new token) from below the
    128-key tile edge to beyond it (edge - 3 -> edge + 7 keys over the rows): a new attention tile goes live, and the O role's
    merge changes its tile count / sweep count (4 tiles per sweep: 512 -> the second sweep).  One row, a pair, and 9 rows = two fours
    + a last chain of one; the rows of 9 beyond the first four and the last sit at other lengths."""
    eng = rig3.eng
    at = [edge - 3, edge - 2, edge - 4, edge - 1]
    lens = at[:n] if n <= 4 else at + [20 + 3 * r for r in range(n - 5)] + [edge - 2]
    xs = [_x(eng, 7000 + edge + r, ln) for r, ln in enumerate(lens)]
    _check(f'context across {edge} keys, {n} rows, {"launches" if shared else "one launch"}', rig3, xs, range(n), shared=shared, one_launch=not shared)


def test_one_row_step_behind_a_1500_token_prompt(dev, rig3):
    """12 attention tiles, merged in three sweeps of four behind the new token's own partial"""
    from cv2amd.llm import LLMEngine
    rig = Rig.__new__(Rig)
    rig.sdr, rig.sd64 = rig3.sdr, rig3.sd64
    rig.eng = LLMEngine(rig3.sdr, dev, max_seqs=1, max_pos=2048, max_out=64, max_prefill_rows=1536)     # (the prompt in one batched prefill)
    _check('one-launch step, 1 row, 1500-token prompt', rig, [_x(rig.eng, 77, 1500)], [0])
    _check('launches, 1 row, 1500-token prompt', rig, [_x(rig.eng, 77, 1500)], [0], shared=True, one_launch=False)


@pytest.mark.parametrize('max_pos,chain', [(1536, True), (4400, False)])
def test_long_context_engines(dev, rig3, max_pos, chain):
    """The engines of test_long_context_attention_splits: larger KV capacities change the launches' key splits (128-key splits with two
    wave groups at 1536, 512-key splits with four groups and a second round of tiles at 4400).  35 tiles x 2 kv heads are more than the
    one-launch step carries (<= 64, csrc/llm.hip: `use_chain` in cv2_llm_create): the 4400 engine has the launches only."""
    from cv2amd.llm import LLMEngine
    rig = Rig.__new__(Rig)
    rig.sdr, rig.sd64 = rig3.sdr, rig3.sd64
    rig.eng = LLMEngine(rig3.sdr, dev, max_seqs=2, max_pos=max_pos, max_out=64)
    assert bool(rig.eng.lib.cv2_llm_one_launch_step(rig.eng.handle)) == chain
    xs = [_x(rig.eng, 400, 300), _x(rig.eng, 401, 41)]
    for shared in ((False, True) if chain else (True,)):
        _check(f'max_pos {max_pos}, 2 rows, {"launches" if shared else "one launch"}', rig, xs, [0, 1], shared=shared, one_launch=not shared)


# ---- rows != slots --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True])
def test_rows_are_not_slots(rig3, shared):
    """cv2_llm_decode_rows over slots 5, 0, 19: row r's logits against the trace of slot slots[r] (its prompt, its ids, its KV rows)"""
    eng = rig3.eng
    slots = [5, 0, 19]
    xs = [_x(eng, 900 + s, ln) for s, ln in zip(slots, (33, 14, 57))]
    _check(f'rows != slots (5, 0, 19), {"launches" if shared else "one launch"}', rig3, xs, slots, shared=shared, one_launch=not shared)


# ---- bistream feeds -------------------------------------------------------------------------------------------------------------
def test_text_block_at_a_position_behind_decode_steps(rig3):
    """cv2_llm_extend_batch at pos0 > 0 (inference_bistream's next text block, llm.py:787-811): after 3 decode steps two slots get
    blocks of 5 and 7 text rows in place of their pending token; the block's last-row logits and the decode steps behind it are held to
    the same bars (stage 4 = the block, stages 5 .. 7 = the steps behind it)."""
    eng = rig3.eng
    g = torch.Generator().manual_seed(5)
    blocks = [eng.text_emb[torch.randint(0, 1000, (k,), generator=g).to(eng.device)].contiguous() for k in (5, 7)]
    xs = [_x(eng, 1200, 26), _x(eng, 1201, 40)]
    _check('text block at pos0 > 0, 2 rows', rig3, xs, [0, 1], steps=6, feed=(3, blocks))


# ---- RAS ------------------------------------------------------------------------------------------------------------------------
def test_ras_sampling_does_not_touch_the_logits(rig3):
    from cv2amd.llm import MODE_RAS
    eng = rig3.eng
    xs = [_x(eng, 1300 + r, ln) for r, ln in enumerate(_lengths(5))]
    _check('RAS, 5 rows, one launch', rig3, xs, range(5), mode=MODE_RAS, seed=0x1234ABCD5)


# ---- 24 layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,shared', [(1, False), (2, False), (9, False), (32, True)])
def test_24_layers(rig24, n, shared):
    eng = rig24.eng
    xs = [_x(eng, 2400 + 50 * n + r, ln) for r, ln in enumerate(_lengths(n, base=10))]
    _check(f'24 layers, {n} rows, {"launches" if shared else "one launch"}', rig24, xs, range(n), shared=shared, one_launch=not shared)


def test_24_layers_heavy_tailed(dev):
    """heavy_tail_llm (massive activations, outlier channels): the model's own distance from fp64 is larger there and gets no absolute
    cap; the ratio bars are the same.  The one-row step and a pair."""
    rig = _make(24, dev, heavy=True, max_seqs=2, max_pos=512, max_out=64)
    for n in (1, 2):
        xs = [_x(rig.eng, 2600 + r, ln) for r, ln in enumerate(_lengths(n, base=10))]
        _check(f'24 layers heavy-tailed, {n} rows, one launch', rig, xs, range(n), cap=False)
