"""Per-slot sampling records on the device (cv2_llm_set_sampling, CV2_ST_SAMP): k_sample alone through the test hook
cv2_llm_debug_sample against the reference fixture and the oracle's sampler functions, then through the engine's request paths.
Run with -m gpu on an MI355X."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EOS = 6561
V = 6564
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'sampler_ras.npz')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def small(dev):
    from cv2amd import synth, weights as W
    from cv2amd.llm import LLMEngine
    sd = synth.make_llm(layers=2)
    return sd, W.round_llm_sd(sd), LLMEngine(sd, dev, max_seqs=32, max_pos=512, max_out=256)


@pytest.fixture(scope='module')
def gd():
    return np.load(GOLDEN)


def _rec(temperature=None, top_p=None, top_k=None, win_size=None, tau_r=None, stream=0):
    from cv2amd.sampling import Sampling
    return Sampling(temperature=temperature, top_p=top_p, top_k=top_k, win_size=win_size, tau_r=tau_r).record(stream=stream)


class Case:
    """what one row of a k_sample launch is given: logits, the decoded tokens so far, step, seed, mode, ignore_eos, record (None: ST_SAMP = 0)"""

    def __init__(self, logits, window, step, seed, ignore_eos, rec=None, mode=1):
        self.logits, self.window, self.step, self.seed, self.ignore_eos, self.rec, self.mode = logits, list(window), step, seed, ignore_eos, rec, mode


def _launch(eng, cases, slots=None):
    """ONE k_sample launch over rows 0 .. n-1 = slots 0 .. n-1 with case i in slot slots[i] (the other slots idle as finished);
    returns [(drawn id, ST_ERR, ST_STEP)] per case"""
    from cv2amd import lib as L
    slots = list(range(len(cases))) if slots is None else slots
    n = max(slots) + 1
    st = torch.zeros(n, L.STATE_STRIDE, dtype=torch.int32)
    st[:, L.ST_DONE] = 1
    toks = torch.zeros(n, eng.max_out, dtype=torch.int32)
    lg = torch.zeros(n, eng.logits.shape[1])
    for c, s in zip(cases, slots):
        wl = len(c.window)
        row = torch.zeros(L.STATE_STRIDE, dtype=torch.int32)
        row[L.ST_POS], row[L.ST_STEP], row[L.ST_NOUT] = 40, c.step, wl
        row[L.ST_MINLEN] = c.step + 1 if c.ignore_eos else 0          # ignore_eos = step < min_len (llm.py:697)
        row[L.ST_MAXLEN], row[L.ST_MODE] = 10_000, c.mode
        row[L.ST_SEED_LO] = (c.seed & 0x7FFFFFFF) - (c.seed & 0x80000000)
        row[L.ST_SEED_HI] = ((c.seed >> 32) & 0x7FFFFFFF) - ((c.seed >> 32) & 0x80000000)
        if c.rec is not None:
            row[L.ST_SAMP] = 1
            eng.set_sampling(s, c.rec)
        st[s] = row
        toks[s, :wl] = torch.tensor(c.window, dtype=torch.int32)
        lg[s, :V] = torch.as_tensor(c.logits, dtype=torch.float32)
    eng.state[:n].copy_(st)
    eng.out_tokens[:n].copy_(toks)
    eng.logits[:n].copy_(lg)
    L.check(eng.lib.cv2_llm_debug_sample(eng.handle, n, L.stream_ptr()))
    got = eng.state[:n].cpu()
    return [(int(got[s, L.ST_LAST]), int(got[s, L.ST_ERR]), int(got[s, L.ST_STEP])) for s in slots]


_CACHE = {}


def _oracle(logits, window, step, seed, ignore_eos, rec, tau_r, ctr0, top_p_scale=1.0, u_scale=1.0):
    """sampling_ids (llm/llm.py:235-250) restated around the oracle's functions with explicit arguments: log_softmax(float32(logits *
    inv_temp)), uniforms = Philox(ctr0, step, trial) under the seed.  The first trial is ras_ids itself; the re-draws repeat its body
    (utils/common.py:111-117) on the row's nucleus_candidates and softmax computed once.  Returns the id, or -1 for the 100-re-draw error."""
    from cv2amd import philox
    from oracle import llm as OL
    top_p, top_k, win = rec['top_p'] * top_p_scale, rec['top_k'], rec['win_size']
    key = (id(logits), rec['inv_temp'])
    if key not in _CACHE:
        z = (torch.as_tensor(logits, dtype=torch.float32) * torch.tensor(rec['inv_temp'], dtype=torch.float32)).to(torch.float32)
        logp = z.log_softmax(dim=-1)
        _CACHE[key] = (logits, logp, logp.softmax(dim=0))
    _, logp, full = _CACHE[key]
    window = list(window)
    trials = 0
    while True:
        u = philox.uniforms(ctr0, step, trials, seed)
        u = (u[0] * u_scale, u[1] * u_scale)
        if trials == 0:
            top = OL.ras_ids(logp, window, u, top_p=top_p, top_k=top_k, win_size=win, tau_r=tau_r)
        else:
            nk = key + (top_p, top_k)
            if nk not in _CACHE:
                _CACHE[nk] = OL.nucleus_candidates(logp, top_p, top_k)
            prob, idx = _CACHE[nk]
            top = idx[OL.multinomial_inv_cdf(prob, u[0])]
            if sum(1 for t in window[-win:] if t == top) >= win * tau_r:
                top = OL.multinomial_inv_cdf(full, u[1])
        if (not ignore_eos) or top != EOS:
            return top
        trials += 1
        if trials > 100:
            return -1


def test_reference_fixture_from_another_slot(small, gd):
    """Every case of tests/golden/sampler_ras.npz in slot 3 with ST_SAMP = 1 and the record {1.0, 0.8, 25, 10, 1.0f, stream 0}: the
    fixture's uniforms were drawn for counter word 0 = 0, so the reference's decision comes out only if the record path equals the
    reference at its constants AND `stream` has replaced the slot.  Modes 1 and 5 (the extract-max path)."""
    sd, sdr, eng = small
    rec = _rec()
    assert rec == dict(inv_temp=1.0, top_p=np.float32(0.8).item(), top_k=25, win_size=10, rep_thr=1.0, stream=0)
    for mode in (1, 5):
        for i in range(len(gd['top'])):
            step, wl = int(gd['step'][i]), int(gd['window_len'][i])
            c = Case(gd['logp'][i], gd['window'][i][:wl].tolist(), step, int(gd['seed'][i]), bool(gd['ignore_eos'][i]), rec, mode)
            (top, err, nstep), = _launch(eng, [c], slots=[3])
            want = int(gd['top'][i])
            if want < 0:
                assert err == 1, f'case {i}, mode {mode}: expected the 100-re-draw error'
            else:
                assert err == 0 and top == want and nstep == step + 1, f'case {i} (kind {int(gd["kind"][i])}, mode {mode}): device {top}, reference {want}'
    eng.park()


def test_slot_independence(small, gd):
    """One launch of 32 rows: identical logits, window, step, seed and record in slots 0, 5, 17, 31 draw the same id; with ST_SAMP = 0 the
    same four draw what Philox keyed by their SLOT predicts (the keying of CV2_ST_SAMP = 0)."""
    from cv2amd import philox
    from oracle import llm as OL
    sd, sdr, eng = small
    same = (0, 5, 17, 31)
    for i, step, seed in ((1, 3, 0xABCDEF0123), (13, 9, 77), (57, 4, 2 ** 63 + 5)):
        wl = int(gd['window_len'][i])
        window, logits = gd['window'][i][:wl].tolist(), gd['logp'][i]
        for seeded in (True, False):
            rec = _rec(stream=2) if seeded else None
            cases = [Case(logits, window, step, seed if s in same else 1000 + s, False, rec if s in same else _rec(stream=s)) for s in range(32)]
            got = _launch(eng, cases)
            ids = [got[s][0] for s in same]
            assert all(got[s][1] == 0 for s in same)
            logp = torch.as_tensor(logits).log_softmax(dim=-1)
            if seeded:
                assert len(set(ids)) == 1, f'row {i}: slots {same} drew {ids}'
                assert ids[0] == OL.ras_ids(logp, window, philox.uniforms(2, step, 0, seed))
            else:
                assert ids == [OL.ras_ids(logp, window, philox.uniforms(s, step, 0, seed)) for s in same]
    eng.park()


def _grid_rows(gd):
    """logits rows and decoded histories of the parameter grid: one fixture row of kinds 0, 1, 2 and 4 with a 64-token history that
    repeats the row's likeliest ids (so that the repetition re-draw happens under some windows and not under others), two rows of
    massively tied values (more than 1024 survivors of the bound: the extract-max path) and one row whose nucleus is the single id EOS
    (drawn when EOS is allowed, the 100-re-draw error when it is not)."""
    g = torch.Generator().manual_seed(2024)
    rows = []
    for i in (0, 12, 28, 56):
        lg = torch.from_numpy(gd['logp'][i]).clone()
        top = lg.topk(4).indices.tolist()
        hist = torch.randint(0, EOS, (64,), generator=g).tolist()
        for j, t in zip((63, 61, 58, 52, 40, 30, 62, 20), (top[0], top[0], top[0], top[0], top[1], top[1], top[2], top[3])):
            hist[j] = t if t < EOS else hist[j]
        rows.append((lg, hist))
    tied = torch.zeros(V)
    tied[5000:5003] = 1.0
    rows.append((tied, [5000, 5001] * 32))
    quant = (torch.randn(V, generator=g) * 2).round() / 2
    rows.append((quant, torch.randint(0, EOS, (64,), generator=g).tolist()))
    single = torch.randn(V, generator=g)
    single[EOS] = 30.0
    rows.append((single, torch.randint(0, EOS, (64,), generator=g).tolist()))
    return rows


GRID = list(itertools.product((0.5, 1, 1.7), (0.3, 0.8, 1.0), (1, 5, 25), ((10, 0.1), (16, 0.2), (64, 0.05)), (False, True)))


def test_parameter_grid_against_the_oracle(small, gd):
    """temperature x top_p x top_k x (win_size, tau_r) x ignore_eos over seven logits rows (1134 cases, 32 per launch, every slot its own
    record): ids and error cases equal the oracle's nucleus_candidates / ras_ids with the same arguments.  The (win_size, tau_r) pairs
    keep win_size * tau_r (1.0, 3.2, 3.2) away from where fp32 and double disagree.
    A mismatch may be left out only as a draw on a cdf boundary: the oracle's own decision changes when its candidate probabilities
    are scaled by 1 +- 1e-6 -- scaling the probabilities is the same as dividing top_p by the factor (the nucleus stops where the
    running sum passes top_p) and, for the mass in front of a cdf step relative to the total, as scaling the uniform; both are tried
    in both directions.  At most 2 % of the grid may be left out that way."""
    sd, sdr, eng = small
    rows = _grid_rows(gd)
    cases, meta = [], []
    for r, (lg, hist) in enumerate(rows):
        for g, (temp, top_p, top_k, (win, tau), ign) in enumerate(GRID):
            rec = _rec(temp, top_p, top_k, win, tau, stream=(7 * r + g) % 11)
            step, seed = 1 + (g % 37), 0x5EED0000 + 131 * r + g
            cases.append(Case(lg, hist, step, seed, ign, rec))
            meta.append((r, temp, top_p, top_k, win, tau, ign))
    assert len(cases) == 7 * 162
    left_out, n_err, n_redraw = [], 0, 0
    for k0 in range(0, len(cases), 32):
        part = cases[k0:k0 + 32]
        got = _launch(eng, part)
        for j, (c, (top, err, _)) in enumerate(zip(part, got)):
            m = meta[k0 + j]
            want = _oracle(c.logits, c.window, c.step, c.seed, c.ignore_eos, c.rec, m[5], c.rec['stream'])
            have = -1 if err == 1 else top
            assert err in (0, 1)
            n_err += want == -1
            if have != want:
                alt = {_oracle(c.logits, c.window, c.step, c.seed, c.ignore_eos, c.rec, m[5], c.rec['stream'], ps, us)
                       for ps, us in ((1 + 1e-6, 1), (1 - 1e-6, 1), (1, 1 + 1e-6), (1, 1 - 1e-6))}
                assert alt != {want}, f'case {m}: device {have}, oracle {want} (no cdf boundary nearby)'
                left_out.append((m, have, want))
    print(f'grid: {len(cases)} cases, {n_err} error cases, left out as cdf-boundary draws: {left_out}')
    assert n_err >= 27                                            # (the single-id EOS row under ignore_eos, at least where top_k = 1)
    assert len(left_out) <= 0.02 * len(cases), left_out
    eng.park()


def test_mixed_rows_equal_their_single_row_launches(small, gd):
    """Eight rows with eight different records in one launch -- two of them ST_SAMP = 0 and one greedy -- each equal to its own
    single-row launch in the same slot."""
    sd, sdr, eng = small
    rows = _grid_rows(gd)
    recs = [_rec(0.5, 0.3, 5, 16, 0.2, stream=9), None, _rec(1.7, 1.0, 25, 64, 0.05, stream=1), _rec(1, 0.8, 1, 10, 0.1, stream=4), None,
            _rec(0.7, 0.9, 12, 3, 0.5, stream=2), _rec(2.0, 0.5, 7, 33, 0.1, stream=0), _rec(1.3, 0.95, 25, 10, 0.1, stream=77)]
    cases = []
    for s, rec in enumerate(recs):
        lg, hist = rows[s % len(rows)]
        cases.append(Case(lg, hist, 2 + s, 900 + s, s % 2 == 1, rec, mode=0 if s == 3 else 1))
    together = _launch(eng, cases)
    alone = [_launch(eng, [c], slots=[s])[0] for s, c in enumerate(cases)]
    assert together == alone
    masked = torch.as_tensor(cases[3].logits).clone()
    masked[EOS] = float('-inf')
    assert together[3][0] == int(masked.argmax())                 # greedy ignores the record (ignore_eos: EOS excluded)
    assert len({t[0] for t in together}) > 2
    eng.park()


def test_set_sampling_range_errors(small):
    from cv2amd import lib as L
    sd, sdr, eng = small
    good = _rec()
    eng.set_sampling(0, good)
    for bad, word in ((dict(top_k=26), 'top_k'), (dict(top_k=0), 'top_k'), (dict(win_size=65), 'win_size'), (dict(win_size=0), 'win_size'),
                      (dict(top_p=0.0), 'top_p'), (dict(top_p=1.5), 'top_p'), (dict(inv_temp=float('inf')), 'inv_temp'),
                      (dict(inv_temp=float('nan')), 'inv_temp'), (dict(inv_temp=0.0), 'inv_temp'), (dict(rep_thr=float('nan')), 'rep_thr')):
        r = L.LlmSampling(**{**good, **bad})
        assert eng.lib.cv2_llm_set_sampling(eng.handle, 0, C.byref(r), L.stream_ptr()) == -1, bad
        assert word in eng.lib.cv2_last_error().decode(), bad
        with pytest.raises(L.Cv2Error):
            eng.set_sampling(0, {**good, **bad})
    r = L.LlmSampling(**good)
    assert eng.lib.cv2_llm_set_sampling(eng.handle, 32, C.byref(r), L.stream_ptr()) == -1
    assert eng.lib.cv2_llm_set_sampling(eng.handle, -1, C.byref(r), L.stream_ptr()) == -1
    torch.cuda.synchronize()


def _requests(n, seed=1986):
    from cv2amd import synth
    reqs = []
    for i in range(n):
        inp = synth.synthetic_inputs(seed=seed + i, text_len=5 + i, prompt_len=9 + 3 * i, prompt_text_len=3 if i % 2 == 0 else 0)
        ptok = inp['prompt_token'] if i % 2 == 0 else torch.zeros(1, 0, dtype=torch.int32)
        reqs.append((inp['text'], inp['prompt_text'], ptok))
    return reqs


def test_seeded_request_through_generate(small):
    """generate(force_len=24): a seeded request alone in slot 0, then as the third of three, then as row 6 of 8 after two shorter
    requests have dropped out of the live-row decode -- the same ids, equal to the oracle's inference under Philox(stream, step, trial)
    with the request's seed at the default constants."""
    from cv2amd import philox
    from cv2amd.llm import MODE_RAS
    from cv2amd.sampling import Sampling
    from oracle import llm as OL
    sd, sdr, eng = small
    seed, stream = 0xC0FFEE1234, 3
    sp = Sampling(seed=seed, stream=stream)
    others = _requests(8, seed=40)
    mine = _requests(1, seed=11)[0]
    want = OL.inference(sdr, *mine, mode='ras', force_len=24, uniforms=lambda step, trial: philox.uniforms(stream, step, trial, seed))
    alone = eng.generate([mine], mode=MODE_RAS, seed=1, force_len=24, sampling=[sp])
    assert int(eng.state[0, 15]) == 1
    assert alone[0] == want
    three = eng.generate([others[0], others[1], mine], mode=MODE_RAS, seed=2, force_len=24, sampling=[None, Sampling(seed=5), sp])
    assert three[2] == want
    assert eng.state[:3, 15].cpu().tolist() == [0, 1, 1]
    reqs = others[:6] + [mine, others[6]]
    fl = [24, 7, 24, 24, 11, 24, 24, 24]
    eight = eng.generate(reqs, mode=[MODE_RAS] * 7 + [0], seed=3, force_len=fl, sync_every=4, sampling=[None] * 6 + [sp, None])
    assert [len(t) for t in eight] == fl and eight[6] == want
    # an unseeded neighbour is still keyed by its slot and the caller's seed: slot 0 of the second run
    assert three[0] == OL.inference(sdr, *others[0], mode='ras', force_len=24, uniforms=lambda step, trial: philox.uniforms(0, step, trial, 2))
    # per-request settings reach the device: top_k = 1 is the per-step argmax of the nucleus until a repetition re-draw
    k1 = eng.generate([mine], mode=MODE_RAS, seed=1, force_len=24, sampling=[Sampling(seed=seed, top_k=1)])[0]
    assert k1 != want
    assert eng.generate([mine], mode=MODE_RAS, seed=1, force_len=24, sampling=[Sampling(greedy=True)])[0] == eng.generate([mine], force_len=24)[0]
    eng.park()


def test_settings_without_a_seed_keep_the_slot_in_the_counter(small):
    """Requests of one generate() call share the caller's seed.  Two of them that carry settings but no seed of their own -- the same
    prompt and text in slots 0 and 1 -- must not consume the same uniforms: their records hold stream = slot, so at the default
    constants each equals the oracle under Philox(slot, step, trial) with the caller's seed, exactly as without a record."""
    from cv2amd import philox
    from cv2amd.llm import MODE_RAS
    from cv2amd.sampling import Sampling
    from oracle import llm as OL
    sd, sdr, eng = small
    mine = _requests(1, seed=11)[0]
    two = eng.generate([mine, mine], mode=MODE_RAS, seed=9, force_len=24, sampling=[Sampling(top_k=25), Sampling(top_k=25)])
    assert eng.state[:2, 15].cpu().tolist() == [1, 1]
    for slot in (0, 1):
        assert two[slot] == OL.inference(sdr, *mine, mode='ras', force_len=24, uniforms=lambda step, trial: philox.uniforms(slot, step, trial, 9)), slot
    assert two[0] != two[1]
    warm = eng.generate([mine, mine, mine], mode=MODE_RAS, seed=9, force_len=24, sampling=[Sampling(temperature=0.8)] * 3, batch_prefill=False)
    assert len({tuple(t) for t in warm}) == 3
    eng.park()


def _bistream_sd():
    """fill / EOS decoder biases under which a SAMPLED bistream call asks for text and ends (the fill id is drawn every few steps, EOS
    now and then; id 6562 never)"""
    from cv2amd import synth
    sd = synth.make_llm(layers=2)
    b = sd['llm_decoder.bias'].clone()
    b[6563] += 8.0
    b[6561] += 6.5
    b[6562] = -30.0
    sd['llm_decoder.bias'] = b
    return sd


def test_seeded_bistream_is_slot_independent_and_equals_the_oracle(dev):
    """new_bistream with a two-block text under a seed: slots 0 and 5 emit the same ids, those of the oracle's inference_bistream under
    Philox(stream, step, trial) with the call's seed."""
    from cv2amd import philox, synth, weights as W
    from cv2amd.llm import LLMEngine, MODE_RAS
    from cv2amd.sampling import Sampling
    from oracle import llm as OL
    sd = _bistream_sd()
    eng = LLMEngine(sd, dev, max_seqs=6, max_pos=512, max_out=256)
    inp = synth.synthetic_inputs(seed=3, text_len=10, prompt_len=15, prompt_text_len=0)
    pieces = lambda: (inp['text'][:, a:b] for a, b in ((0, 5), (5, 10)))      # noqa: E731
    seed, stream = 0xB15712EA, 1
    want, want_all = OL.inference_bistream(W.round_llm_sd(sd), list(pieces()), inp['prompt_text'], inp['prompt_token'], mode='ras',
                                           uniforms=lambda step, trial: philox.uniforms(stream, step, trial, seed), max_steps=250)
    assert len(want) >= 8 and 6563 in want_all
    for slot in (0, 5):
        got = list(eng.bistream(slot, pieces(), inp['prompt_text'], inp['prompt_token'], mode=MODE_RAS, seed=99,
                                sampling=Sampling(seed=seed, stream=stream)))
        assert got == want, f'slot {slot}'
        assert int(eng.state[slot, 15]) == 1
    # settings without a seed: the call runs under its caller's seed and keeps the slot in the counter, as without a record
    plain = {}
    for slot in (0, 5):
        plain[slot] = list(eng.bistream(slot, pieces(), inp['prompt_text'], inp['prompt_token'], mode=MODE_RAS, seed=99, sampling=Sampling(top_k=25)))
        assert int(eng.state[slot, 15]) == 1
    assert plain[0] != plain[5]
    want5, _ = OL.inference_bistream(W.round_llm_sd(sd), list(pieces()), inp['prompt_text'], inp['prompt_token'], mode='ras',
                                     uniforms=lambda step, trial: philox.uniforms(5, step, trial, 99), max_steps=250)
    assert plain[5] == want5
    eng.park()
