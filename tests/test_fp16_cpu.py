"""CPU tests of the fp16 flow operands (no GPU): the fp16 weight packing, the --verify fp16 range report, the ABI revision of the C library."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_f16_is_the_bf16_permutation_with_fp16_bit_patterns():
    from cv2amd import weights as W
    g = torch.Generator().manual_seed(3)
    for n, k in ((16, 32), (20, 64), (80, 256), (1024, 320)):              # N = 20 / 80: padded to 32 / 80 rows of 16
        w = torch.randn(n, k, generator=g) * 4
        w[0, 0], w[-1, -1], w[n // 2, 1] = 1e6, -1e6, 3e-9               # saturated, saturated, flushed to zero
        npad = (n + 15) // 16 * 16
        pb = W.pack_bf16(w)
        ph = W.pack_f16(w)
        assert ph.dtype == pb.dtype == torch.int16 and ph.shape == pb.shape == (npad * k,)
        probe = torch.zeros(npad, k)
        ref = torch.empty(npad * k, dtype=torch.int16)
        wp = torch.zeros(npad, k)
        wp[:n] = w
        wh = wp.clamp(-65504, 65504).half().view(torch.int16).reshape(-1)          # padding rows: fp16 zeros
        # locate every element through pack_bf16 of one-hot probes, a 16 x 32 block at a time (the layout is block-local)
        for r in range(16):
            for c in range(32):
                probe.zero_()
                probe[r::16, c::32] = 1.0
                pos = (W.pack_bf16(probe) != 0).nonzero().reshape(-1)
                rows = torch.arange(r, npad, 16).repeat_interleave(k // 32)
                cols = torch.arange(c, k, 32).repeat(npad // 16)
                ref[pos] = wh[(rows * k + cols)]
        assert torch.equal(ph, ref)
    assert W.f16_round(torch.tensor([1e6, -1e6, 3e-9, 1.0])).tolist() == [65504.0, -65504.0, 0.0, 1.0]


def test_verify_reports_the_fp16_range_of_the_flow_weights():
    from cv2amd import checkpoint as CK, synth
    sd = synth.make_flow()
    r0 = CK.fp16_range(sd)
    assert r0['n_over'] == 0 and 0 < r0['max_abs'] < 65504 and r0['n'] > 1e6         # (random weights: a few may sit below 2^-24 already)
    k1, k2 = 'decoder.estimator.mid_blocks.3.1.0.ff.net.2.weight', 'encoder.encoders.0.self_attn.linear_q.weight'
    sd = dict(sd)
    sd[k1] = sd[k1].clone()
    sd[k1][0, :3] = torch.tensor([7e4, -1e5, 65504.0])                  # two above 65504 (65504 itself is representable)
    sd[k2] = sd[k2].clone()
    sd[k2][1, :4] = torch.tensor([1e-8, -2e-8, 0.0, 2.0 ** -24])          # two nonzero below 2^-24 (zero and 2^-24 itself do not flush)
    sd['input_embedding.weight'] = sd['input_embedding.weight'].clone() * 1e6     # fp32 VALU table, not a matrix operand: not counted
    r = CK.fp16_range(sd)
    assert (r['n_over'], r['n_flush'] - r0['n_flush'], r['max_abs'], r['max_key']) == (2, 2, 1e5, k1)
    assert r['over_keys'] == [k1] and k2 in r['flush_keys'] and set(r['flush_keys']) - set(r0['flush_keys']) <= {k2}
    text = '\n'.join(CK.fp16_report(sd))
    assert '2 above 65504' in text and '{} nonzero below 2^-24'.format(r['n_flush']) in text and 'fp16 OVERFLOW ' + k1 in text


def test_abi_revision_3_and_the_fp16_gemm_hook():
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from cv2amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'cv2_amd.h')).read()
    assert int(re.search(r'#define\s+CV2_ABI_VERSION\s+(\d+)', hdr).group(1)) == 3 == L.ABI_VERSION
    cdll = ctypes.CDLL(L.LIB_PATH)
    assert cdll.cv2_version() == 3
    assert re.search(r'\bint cv2_gemm_f16\(', hdr) and 'cv2_gemm_f16' in L.EXPORTS and hasattr(cdll, 'cv2_gemm_f16')
    assert re.search(r'int32_t operands;', hdr) and '#define CV2_OPERANDS_FP16 1' in hdr


def test_flow_engine_refuses_an_unknown_operand_format():
    from cv2amd.flow import FlowEngine
    with pytest.raises(ValueError, match="operands must be 'bf16' or 'fp16'"):
        FlowEngine({}, 'cpu', operands='fp8')
