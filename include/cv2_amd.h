/* cv2_amd.h — C ABI of libcv2amd.so: the MI355X (gfx950) hot path of CosyVoice2-0.5B-EU synthesis.
 *
 * Drop-in boundary.  The reference is pure Python; the seams these entry points replace are
 *   LLM   : Qwen2LM.inference / inference_wrapper            cosy_repo/cosyvoice/llm/llm.py:575-719
 *           (precedent for an external engine: the vLLM branch, llm.py:651-680 — add_request(prompt_embeds),
 *            step(), queue of ids)
 *   Flow  : CausalMaskedDiffWithXvec.inference               cosy_repo/cosyvoice/flow/flow.py:235-283
 *           ConditionalCFM.forward_estimator (TensorRT seam) cosy_repo/cosyvoice/flow/flow_matching.py:125-150
 *   HiFT  : HiFTGenerator.inference                          cosy_repo/cosyvoice/hifigan/generator.py:570-582
 *   fade  : fade_in_out                                      cosy_repo/cosyvoice/utils/common.py:142-150
 *
 * Conventions: plain pointers and sizes only; every tensor argument is a DEVICE pointer owned by the caller
 * (the Python host allocates with torch); the library never frees caller memory and never returns owned
 * memory except opaque handles; all launches go to the hipStream_t passed in (as void*); return 0 on success,
 * negative on error with a message available from cv2_last_error().
 */
#ifndef CV2_AMD_H
#define CV2_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* cv2_last_error(void);
/* ABI revision of the structs and entry points below; bumped whenever a struct's layout or a signature changes (2: cv2_hift_weights gained
 * sd_conv[3] in front of src_rb; 3: cv2_flow_dims gained `operands`, cv2_gemm_f16 was added).  cv2_version() returns the library's; a binding built against another revision must refuse to run
 * (cv2amd/lib.py does) -- a stale libcv2amd.so would otherwise misread every pointer behind the changed field without any error. */
#define CV2_ABI_VERSION 3
int cv2_version(void);

/* ------------------------------------------------------------------------------------------------
 * Stage 1 — Qwen2 speech-token LM (replaces llm.py:575-719; HF Qwen2ForCausalLM call sites llm.py:107-117)
 *
 * Weight layout in HBM ("packed"): a [N,K] bf16 matrix is stored as 1 KiB blocks in MFMA 16x16x32 operand
 * order: block (nt, ks) holds rows 16nt..16nt+15, columns 32ks..32ks+31; within a block lane l (0..63) owns
 * 8 consecutive bf16 of row 16nt + (l & 15), columns 32ks + 8(l >> 4) .. +7.  Blocks are ordered [nt][ks].
 * A wave streams one row tile with perfectly sequential 1 KiB loads.  cv2amd/weights.py builds this layout.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cv2_llm cv2_llm;

typedef struct {
    int32_t hidden;     /* 896  */
    int32_t inter;      /* 4864 */
    int32_t layers;     /* 24   */
    int32_t n_q;        /* 14 query heads */
    int32_t n_kv;       /* 2 kv heads     */
    int32_t vocab;      /* 6564 = speech_token_size + 3 (llm.py:392-397) */
    int32_t vocab_pad;  /* vocab rounded up to 16 */
    int32_t eos;        /* 6561 */
    int32_t max_seqs;   /* sequence slots (<= 32) */
    int32_t max_pos;    /* KV capacity per sequence */
    int32_t max_out;    /* capacity of out_tokens per sequence */
    float rms_eps;      /* 1e-6 */
    int32_t max_prefill_rows; /* capacity of cv2_llm_prefill_batch in prompt rows (0: only the 32-row cv2_llm_prefill) */
    /* ras_sampling constants (utils/common.py:111-139, values from conf/cosyvoice2.yaml:33-37); top_k == 0 selects 0.8 / 25 / 10 / 0.1 */
    float top_p;        /* nucleus mass */
    int32_t top_k;      /* nucleus size, 1..25 */
    int32_t win_size;   /* repetition window, <= 64 */
    float tau_r;        /* full-vocabulary re-draw when the drawn id occurs >= win_size * tau_r times in the window */
} cv2_llm_dims;

typedef struct {
    const uint16_t* wqkv;  /* packed [(n_q+2n_kv)*64, hidden]: q rows, then k rows, then v rows */
    const float* bqkv;     /* [(n_q+2n_kv)*64] */
    const uint16_t* wo;    /* packed [hidden, n_q*64] */
    const uint16_t* wgu;   /* packed [2*inter, hidden]; row tiles interleaved: gate tile i, up tile i, ... */
    const uint16_t* wdown; /* packed [hidden, inter] */
    const float* ln1;      /* input_layernorm.weight [hidden] */
    const float* ln2;      /* post_attention_layernorm.weight [hidden] */
} cv2_llm_layer;

typedef struct {
    const cv2_llm_layer* layers; /* HOST array of `layers` entries holding device pointers */
    const float* final_norm;     /* [hidden] */
    const uint16_t* wdec;        /* packed [vocab_pad, hidden] (llm_decoder, zero rows beyond vocab) */
    const float* bdec;           /* [vocab_pad] */
    const float* speech_emb;     /* [vocab, hidden] fp32 (speech_embedding.weight) */
    const float* rope_cos;       /* [max_pos, 32] cos(pos * theta^(-2i/64)) — built on the host as HF does */
    const float* rope_sin;       /* [max_pos, 32] */
} cv2_llm_weights;

/* per-sequence state, int32[CV2_LLM_STATE_STRIDE] per slot, device memory owned by the caller */
enum {
    CV2_ST_POS = 0,      /* next KV position */
    CV2_ST_STEP = 1,     /* loop index i of inference_wrapper (llm.py:684) */
    CV2_ST_NOUT = 2,     /* emitted tokens so far */
    CV2_ST_DONE = 3,     /* 1 once EOS was drawn or max_len reached */
    CV2_ST_MINLEN = 4,   /* int(text_len * min_token_text_ratio) */
    CV2_ST_MAXLEN = 5,   /* int(text_len * max_token_text_ratio) */
    CV2_ST_MODE = 6,     /* 0 greedy (harness-defined), 1 RAS with the constants of cv2_llm_dims (or the slot's record, CV2_ST_SAMP) */
    CV2_ST_FORCE = 7,    /* 1: synthetic-weights mode, ids >= eos never drawn (fixed decode length) */
    CV2_ST_SEED_LO = 8,
    CV2_ST_SEED_HI = 9,
    CV2_ST_ERR = 10,     /* 1: sampler exhausted 100 EOS re-draws (RuntimeError in llm.py:249); 2: bistream drew a special id it must
                          * not ("should not get token", ValueError in llm.py:809, 829) */
    CV2_ST_LAST = 11,    /* last drawn id */
    CV2_ST_BIMODE = 12,  /* inference_bistream (llm.py:721-834): 0 unistream, 1 text still expected, 2 final decode */
    CV2_ST_NEXTFILL = 13,/* next_fill_index of llm.py:783 (-1: none yet); counts entries of out_tokens incl. fill ids */
    CV2_ST_WAIT = 14,    /* 1: the slot stopped on the fill id (eos + 2) and waits for cv2_llm_extend with the next text block */
    CV2_ST_SAMP = 15,    /* 0: the sampler constants of cv2_llm_dims and Philox counter word 0 = the slot; 1: the slot's cv2_llm_sampling record
                          * (cv2_llm_set_sampling) */
    CV2_LLM_STATE_STRIDE = 16
};

typedef struct {
    int32_t* state;      /* [max_seqs][CV2_LLM_STATE_STRIDE] */
    int32_t* out_tokens; /* [max_seqs][max_out] emitted speech tokens */
    float* logits;       /* [32][vocab_pad] last step's llm_decoder output (for parity tests) */
} cv2_llm_io;

size_t cv2_llm_workspace_bytes(const cv2_llm_dims* dims);
int cv2_llm_create(const cv2_llm_dims* dims, const cv2_llm_weights* w, const cv2_llm_io* io, void* workspace,
                   size_t workspace_bytes, cv2_llm** out);
int cv2_llm_destroy(cv2_llm* h);
/* Step 0 of inference_wrapper for slot `seq`: run the backbone over prompt_embeds [len, hidden] fp32
 * (= lm_input of llm.py:641, the vLLM seam's prompt_embeds), fill the KV cache, draw the first token.
 * state[seq] must have been initialised by the caller (pos = step = nout = done = 0, lens, mode, seed). */
int cv2_llm_prefill(cv2_llm* h, int32_t seq, const float* prompt_embeds, int32_t len, void* stream);
/* Step 0 for several slots at once through the MFMA GEMM path (operand split hi + lo): embeds = the prompts' rows
 * concatenated, fp32 [sum(lens)][hidden] on the device; slots / lens are HOST arrays of n entries.  state[slot] must be
 * initialised like for cv2_llm_prefill.  Weights are streamed once for all rows. */
int cv2_llm_prefill_batch(cv2_llm* h, int32_t n, const int32_t* slots, const int32_t* lens, const float* embeds, void* stream);
/* inference_bistream (llm.py:787-811, 817-832): `len` further input rows for slot `seq` at KV positions pos0 .. pos0 + len - 1
 * (embeds fp32 [len][hidden], device), then one draw from the last row under state[seq] (CV2_ST_BIMODE, CV2_ST_NEXTFILL).  In
 * bistream modes out_tokens receives EVERY drawn id (fill and EOS included), as the reference's out_tokens list does. */
int cv2_llm_extend(cv2_llm* h, int32_t seq, const float* embeds, int32_t len, int32_t pos0, void* stream);
/* The same for n slots in one pass over the weights (the matrix-core path of cv2_llm_prefill_batch): the text blocks that concurrent
 * inference_bistream calls (cli/model.py:120-128 x the streams of BASELINE configs[4]) are waiting to feed.  slots / lens / pos0 are HOST
 * arrays of n entries (distinct slots), embeds = the slots' rows concatenated, fp32 [sum(lens)][hidden] on the device; one draw per slot
 * from its last row under state[slot].  sum(lens) rounded up to 128 must fit max_prefill_rows. */
int cv2_llm_extend_batch(cv2_llm* h, int32_t n, const int32_t* slots, const int32_t* lens, const int32_t* pos0, const float* embeds, void* stream);
/* n_steps iterations of the decode loop for slots 0..n_seqs-1 in lock step (one hipGraph replay per step);
 * finished slots idle.  No host synchronisation inside.
 * Up to 24 sequences: a step is ONE launch followed by the sampler -- k_step (csrc/chain.h: every layer's Q / attention / O / gate-up /
 * down roles and the head as blocks of one grid in dependency order, activations handed over as epoch-tagged granules) at one row;
 * k_step_rows<2> / k_step_rows<4> at 2 .. 8 / 9 .. 24 rows (the rows in pairs / fours as columns of the blocks' MFMA operands, one chain of blocks per
 * group; 3 rows: one chain per row).  From 25 rows on, and whenever the environment variable CV2_LLM_CHAIN=0 is set at create, a step is
 * five to seven launches per layer.  CV2_ST_ERR = 3 reports a hand-off that timed out: that step (and every later step of the call)
 * commits nothing -- state, tokens and the KV positions are the ones before it -- so the caller clears the flag and repeats the steps
 * with CV2_DECODE_SHARED (the launches). */
int cv2_llm_decode(cv2_llm* h, int32_t n_seqs, int32_t n_steps, void* stream);
/* The same with flags.  CV2_DECODE_SHARED: other streams' kernels run beside these steps (the streaming scheduler overlaps a decode
 * burst with the previous chunk's flow + HiFT): use the launches even at one row -- k_step's resident polling waves cost the
 * neighbours more than they save here (one stream: 34 -> 40 ms between chunks with k_step beside the chunk work). */
#define CV2_DECODE_SHARED 1
int cv2_llm_decode_ex(cv2_llm* h, int32_t n_seqs, int32_t n_steps, int32_t flags, void* stream);
/* n_steps of the decode loop over the LIVE slots only: row r of every step serves slot slots[r] (host array, n_rows distinct slot
 * ids, copied before the call returns).  A batch of llm.py:649-719 generations ends request by request; the scheduler drops the
 * finished slots from the list at every poll, so a step costs what its live rows cost (the slots' state, caches and results are
 * the ones cv2_llm_decode uses: the two calls may alternate on the same slots). */
int cv2_llm_decode_rows(cv2_llm* h, const int32_t* slots, int32_t n_rows, int32_t n_steps, int32_t flags, void* stream);
/* 1 when decode steps of up to 24 rows of this engine run as one launch (k_step / k_step_rows), 0 when they run as launches (dims
 * outside k_step's limits, or CV2_LLM_CHAIN=0). */
int cv2_llm_one_launch_step(const cv2_llm* h);
/* test hook: from now on Q-role block `q_block` of layer `layer` of every one-launch step does not publish its results (layer < 0: off; the
 * same (layer, block) key in every one-launch form), so the blocks behind it end in their bounded waits and EVERY row of the block's chain
 * reports CV2_ST_ERR = 3 without committing anything. */
int cv2_llm_debug_skip_publish(cv2_llm* h, int32_t layer, int32_t q_block);
/* test / diagnostic hook: device addresses of the decode workspaces and the granule layout (16 values; tools/dbg_chain_vals.py) */
int cv2_llm_debug_ptrs(cv2_llm* h, uint64_t* out);
/* test hook: ONE sampler launch (k_sample) over slots 0 .. n_rows - 1 from whatever the caller has put into logits[row], state[slot] and
 * out_tokens[slot] -- TransformerLM.sampling_ids + ras_sampling (llm/llm.py:235-250, utils/common.py:111-139) on their own, so that
 * tests/golden/sampler_ras.npz (decisions of the reference's functions under a committed table of uniforms = this sampler's Philox draws)
 * can be replayed on the device.  Updates the slots exactly as a decode step's draw does. */
int cv2_llm_debug_sample(cv2_llm* h, int32_t n_rows, void* stream);

/* Sampler settings of ONE request (an extension: the reference has one ras_sampling configuration per model and the process-wide torch RNG).
 * The engine keeps one record per slot in its workspace (max_seqs records at an address fixed at create: captured decode steps stay valid);
 * k_sample uses the record of a slot whose state row has CV2_ST_SAMP = 1 and the constants of cv2_llm_dims otherwise, row by row of one
 * launch.  With a record, in a RAS mode (CV2_ST_MODE 1, test mode 5; greedy draws nothing and ignores it):
 *   z[i] = logits[i] * inv_temp, ONE fp32 multiply rounded on its own (inv_temp = 1.0f: the identity), then the pipeline of CV2_ST_SAMP = 0 on z -- the
 *   step-0 / forced-length / ignore_eos masks, log-softmax, the nucleus under top_p / top_k by the running fp32 sum, the repetition count over
 *   the last win_size tokens against rep_thr, the full-vocabulary re-draw, up to 100 EOS re-draws (CV2_ST_ERR = 1);
 *   every Philox draw has counter (stream, step, trial, 0) and key CV2_ST_SEED_LO / HI: the uniforms of a request are a function of
 *   (seed, stream, step, trial) and not of the slot, the row or the other rows of the launch.  Requests that share one seed must differ in
 *   `stream`: a caller that gives a request settings but no seed of its own writes stream = the slot, as with CV2_ST_SAMP = 0.
 * Unistream, bistream and prefill draws alike.  At create every record holds the engine's constants with stream = its slot.
 * cv2_llm_set_sampling checks the ranges (-1 and cv2_last_error otherwise) and writes the record in stream order (a one-block kernel that
 * takes it by value): the caller writes it ahead of the state row and the prefill on the same stream.  Adding this entry point and state
 * word changed no struct and no signature: CV2_ABI_VERSION stays. */
typedef struct {
    float    inv_temp;   /* float32(1 / temperature), formed on the host; finite, > 0 */
    float    top_p;      /* (0, 1] */
    int32_t  top_k;      /* 1 .. 25 */
    int32_t  win_size;   /* 1 .. 64 */
    float    rep_thr;    /* (float)win_size * tau_r, the fp32 product cv2_llm_create forms for the engine's constants; >= 0 */
    uint32_t stream;     /* Philox counter word 0 in place of the slot */
    int32_t  reserved[2];
} cv2_llm_sampling;                                                  /* 32 bytes */
int cv2_llm_set_sampling(cv2_llm* h, int32_t slot, const cv2_llm_sampling* s /* host */, void* stream);

/* Stand-alone skinny GEMM used by the LLM (exported for unit tests and for the flow time-MLP):
 * out[r][n] = sum_k W[n][k] x[r][k] (+bias[n]); rows <= 32; W packed; K % 32 == 0; N % 16 == 0. */
int cv2_skinny_gemm(const uint16_t* w_packed, const float* bias, const float* x, float* out, int32_t rows,
                    int32_t n, int32_t k, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Generic bf16 MFMA GEMM (exported for unit tests): out[m][n] = sum_k A[m][k] W[n][k] (+bias[n]).
 * A row-major bf16 [M][lda] (M % 128 == 0, K % 64 == 0), W packed (above), out fp32 [M][ldo], N % 128 == 0.
 * ---------------------------------------------------------------------------------------------- */
int cv2_gemm_bf16(const uint16_t* a, int64_t lda, const uint16_t* w_packed, const float* bias, float* out, int64_t ldo,
                  int32_t m, int32_t n, int32_t k, void* stream);
/* The same on fp16 operands (A and W hold fp16 bit patterns, W in the same packed order): the GEMM of an fp16 flow engine. */
int cv2_gemm_f16(const uint16_t* a, int64_t lda, const uint16_t* w_packed, const float* bias, float* out, int64_t ldo,
                 int32_t m, int32_t n, int32_t k, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stage 2 — token -> mel (replaces CausalMaskedDiffWithXvec.inference, cosyvoice/flow/flow.py:235-283, and
 * everything below it: UpsampleConformerEncoder.forward transformer/upsample_encoder.py:243-306,
 * CausalConditionalCFM.forward / solve_euler flow/flow_matching.py:200-225,71-123,
 * CausalConditionalDecoder.forward flow/decoder.py:405-494).
 *
 * Linear / Conv1d weights are 16-bit in the packed layout above, in the engine's operand format (cv2_flow_dims.operands:
 * bf16, or fp16 rounded to nearest even and saturated to +-65504); a Conv1d weight [C_out][C_in][k] is packed as the
 * [C_out][k*C_in] matrix with column index tap*C_in + c_in (time-major activations make the tap window contiguous).
 * Biases, LayerNorm parameters, embeddings stay fp32.  Every matrix-product operand of the engine -- weights, the activations
 * fed to GEMMs and convolutions, attention q / k / v, softmax probabilities, the stream caches' keys / values -- is held in
 * that format; accumulation, LayerNorm, softmax statistics, the residual stream, the Euler state and the mel stay fp32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cv2_flow cv2_flow;

typedef struct { const uint16_t* w; const float* b; } cv2_lin;      /* packed 16-bit weight in the engine's operand format, fp32 bias (may be NULL) */
typedef struct { const float* g; const float* b; } cv2_ln;

typedef struct {            /* ConformerEncoderLayer (transformer/encoder_layer.py:160-236) */
    cv2_ln norm_mha, norm_ff;
    cv2_lin qkv;            /* rows [Wq; Wq; Wk; Wv] (2048 x 512), bias [bq + pos_bias_u; bq + pos_bias_v; bk; bv] */
    cv2_lin pos;            /* linear_pos 512 -> 512, no bias */
    cv2_lin out;            /* linear_out */
    cv2_lin w1, w2;         /* feed_forward 512 -> 2048 -> 512 */
} cv2_conformer;

typedef struct {            /* matcha BasicTransformerBlock (matcha/models/components/transformer.py:243-316) */
    cv2_ln norm1, norm3;
    cv2_lin qkv;            /* rows [to_q; to_k; to_v] (1536 x 256), no bias */
    cv2_lin out;            /* to_out.0 512 -> 256 */
    cv2_lin ff1, ff2;       /* 256 -> 1024 (GELU) -> 256 */
} cv2_tblock;

typedef struct {            /* CausalResnetBlock1D (flow/decoder.py:65-85, matcha decoder.py:46-61) */
    cv2_lin conv1;          /* [256][3*C_in] */
    cv2_ln ln1;
    cv2_lin mlp;            /* Linear 1024 -> 256 applied to Mish(time embedding) */
    cv2_lin conv2;          /* [256][3*256] */
    cv2_ln ln2;
    cv2_lin res;            /* res_conv 1x1: [256][C_in] */
} cv2_resnet;

typedef struct {
    cv2_resnet rn;
    cv2_tblock tb[4];
    cv2_lin tail;           /* down/up CausalConv1d(256,256,3); w == NULL for mid blocks */
} cv2_unet_block;

typedef struct {
    const float* input_embedding;   /* [6561][512] */
    const float* spk_w;             /* spk_embed_affine_layer.weight [80][192] fp32 */
    const float* spk_b;             /* [80] */
    cv2_lin embed; cv2_ln embed_ln;             /* encoder.embed.out.{0,1} */
    cv2_lin pre1, pre2;                         /* pre_lookahead conv1 [512][4*512], conv2 [512][3*512] */
    cv2_conformer enc[6];
    cv2_lin up_conv;                            /* encoder.up_layer.conv [512][5*512] */
    cv2_lin up_embed; cv2_ln up_embed_ln;
    cv2_conformer up[4];
    cv2_ln after_norm;
    cv2_lin enc_proj;                           /* encoder_proj 512 -> 80, rows padded to 128 */
    cv2_lin time1, time2;                       /* time_mlp linear_1 (320 -> 1024), linear_2 (1024 -> 1024) */
    cv2_unet_block down, mid[12], up_blk;
    cv2_lin final_conv; cv2_ln final_ln;        /* final_block */
    cv2_lin final_proj;                         /* 256 -> 80, rows padded to 128 */
    const float* rand_noise;                    /* [15000][80] fp32: flow_matching.py:197-198 noise, time-major */
} cv2_flow_weights;

typedef struct {
    int32_t max_rows;       /* capacity: packed mel-rate rows (sum over sequences of the padded lengths) */
    int32_t max_seqs;       /* sequences per call incl. the CFG twins (2 x utterances) */
    int32_t max_len;        /* longest single sequence in mel frames */
    int32_t n_timesteps;    /* Euler steps (10) */
    float cfg_rate;         /* inference_cfg_rate (0.7) */
    int32_t operands;       /* CV2_OPERANDS_BF16 = 0, CV2_OPERANDS_FP16 = 1: the 16-bit format of every matrix operand, fixed at
                               cv2_flow_create (one engine holds one packed weight set; the weights must be packed in this format) */
} cv2_flow_dims;
#define CV2_OPERANDS_BF16 0
#define CV2_OPERANDS_FP16 1

size_t cv2_flow_workspace_bytes(const cv2_flow_dims* d);
int cv2_flow_create(const cv2_flow_dims* d, const cv2_flow_weights* w, void* workspace, size_t workspace_bytes,
                    void* stream, cv2_flow** out);
int cv2_flow_destroy(cv2_flow* h);

/* One batch of utterances through flow.inference (flow.py:235-283).  For utterance u (all pointers DEVICE):
 *   tokens[u]       int32 [n_tok[u]]     prompt tokens followed by generated tokens (flow.py:252)
 *   prompt_feat[u]  fp32  [n_prompt_feat[u]][80]   prompt mel, time-major (the reference's prompt_feat[0])
 *   embedding[u]    fp32  [192]
 *   mel_out[u]      fp32  [80][mel_len2[u]] channel-major like the reference's return value,
 *                   mel_len2 = 2 * (n_tok - 3 * !finalize) - n_prompt_feat
 * streaming: chunk-causal attention masks (static chunk 25 tokens / 50 frames); finalize == 0: the last 3 tokens are
 * look-ahead context (flow.py:260-263). */
typedef struct {
    const int32_t* tokens; int32_t n_tok;
    const float* prompt_feat; int32_t n_prompt_feat;
    const float* embedding;
    float* mel_out;
} cv2_flow_utt;
int cv2_flow_inference(cv2_flow* h, const cv2_flow_utt* utts, int32_t n_utts, int32_t streaming, int32_t finalize, void* stream);

/* Streaming calls with a per-stream cache.  The reference's token2wav re-runs flow.inference over the WHOLE prefix for every chunk
 * (cli/model.py:351-381, 300-311) and keeps mel[token_offset * 2:].  With streaming masks the estimator is chunk-causal (flow/decoder.py:
 * 439-441: static chunk of 50 frames; every convolution is causal), so the frames of finished chunks never change: this entry point
 * computes only the frames the cache does not hold yet and returns exactly those the recompute would have produced for them.  The encoder
 * (transformer/upsample_encoder.py:243-306) is chunk-causal in the same way; its per-layer keys / values and convolution tails live in the same
 * cache, so a call's encoder pass covers the new tokens only (CV2_ENC_CACHE=0: recompute the prefix, diagnostics).
 *   cache         device memory of cv2_flow_cache_bytes(h, cache_frames) bytes, ZERO-initialised by the caller before the first call of a
 *                 stream, owned by the caller (one per stream); cache_frames = a multiple of 64 >= the longest prefix in frames
 *   n_cached      frames the cache holds = 2 * (n_tok - 3) of the stream's previous (non-final) call, 0 on the first call; a multiple of 50
 *   gen           0 on the first call, +1 after every SUCCESSFUL call (the convolution tails are double-buffered on it, so a failed
 *                 call can be repeated)
 * utts[u] as for cv2_flow_inference (tokens = the whole prefix), except
 *   mel_out[u]    fp32 [80][n] with n = 2 * (n_tok - 3 * !finalize) - max(n_cached, n_prompt_feat): the frames after the cached ones
 * A non-final call must end on a chunk boundary (2 * (n_tok - 3) % 50 == 0), as the reference's hop alignment guarantees
 * (cli/model.py:357-360). */
typedef struct { void* cache; int32_t cache_frames; int32_t n_cached; int32_t gen; } cv2_flow_cache_ref;
size_t cv2_flow_cache_bytes(const cv2_flow* h, int32_t cache_frames);
int cv2_flow_inference_chunk(cv2_flow* h, const cv2_flow_utt* utts, const cv2_flow_cache_ref* refs, int32_t n_utts, int32_t finalize,
                             void* stream);
/* The first n_frames (whole chunks of 50) of one cache and its convolution tails into another cache (other capacity allowed): a stream
 * whose prompt (tokens, mel, speaker embedding) another call has already run starts from that call's cache — n_cached = n_frames and the
 * same `gen` as the source.  The source must hold exactly n_frames (its tails belong to that position). */
int cv2_flow_cache_copy(const cv2_flow* h, const void* src, int32_t src_frames, void* dst, int32_t dst_frames, int32_t n_frames, void* stream);

/* Solver settings of a call (an extension: the reference passes n_timesteps to CausalConditionalCFM.forward and reads inference_cfg_rate
 * inside solve_euler, flow_matching.py:71-123; cv2_flow_dims fixes both per engine).  One record per utterance:
 *   n_timesteps   Euler steps 1 .. 31 on the cosine grid t_span = 1 - cos(linspace(0, 1, n + 1) * pi / 2); <= 0: the engine's
 *   cfg_rate      classifier-free-guidance rate, finite and >= 0 (at 0 both branches still run); < 0: the engine's
 * The update of a step is x + dt * ((1 + cfg_rate) * v_cond - cfg_rate * v_uncond) with the utterance's own rate, so utterances with
 * different rates share a launch.  ALL records of one call must resolve to the same step count (the estimator's time embedding and the
 * number of launches are the call's); a call that mixes them, or carries a value out of range, returns -1 before any launch.  The time
 * table of a step count other than the engine's is built at its first use and stays resident in the workspace.  solver == NULL is
 * cv2_flow_inference / cv2_flow_inference_chunk: the same launches with the same arguments.
 * A stream's cache is laid out for its step count (slots [n][56], convolution tails [2][n][31]) and holds keys / values made on that t
 * grid under that guidance rate: size it with cv2_flow_cache_bytes_ex, copy it with cv2_flow_cache_copy_ex and keep one (n_timesteps,
 * cfg_rate) for all calls of a stream -- the entry points cannot tell what a cache was filled with.  n_timesteps <= 0 there: the engine's.
 * cv2_flow_schedule writes the t and dt of the n steps as the Euler loops walk them (host arithmetic, no device needed).
 * Adding these entry points changed no struct and no signature: CV2_ABI_VERSION stays. */
typedef struct { int32_t n_timesteps; float cfg_rate; } cv2_flow_solver;
int cv2_flow_inference_ex(cv2_flow* h, const cv2_flow_utt* utts, const cv2_flow_solver* solver, int32_t n_utts, int32_t streaming,
                          int32_t finalize, void* stream);
int cv2_flow_inference_chunk_ex(cv2_flow* h, const cv2_flow_utt* utts, const cv2_flow_cache_ref* refs, const cv2_flow_solver* solver,
                                int32_t n_utts, int32_t finalize, void* stream);
size_t cv2_flow_cache_bytes_ex(const cv2_flow* h, int32_t cache_frames, int32_t n_timesteps);
int cv2_flow_cache_copy_ex(const cv2_flow* h, const void* src, int32_t src_frames, void* dst, int32_t dst_frames, int32_t n_frames,
                           int32_t n_timesteps, void* stream);
int cv2_flow_schedule(int32_t n_timesteps, float* t_out, float* dt_out);

/* Test hook: 1 or -1 = the default forms of the estimator attention (key / value tiles by LDS DMA: one key group from 512 blocks of
 * 8 heads x 64 query rows on -- 257 for a full-context call without cache --, four key groups below), 0 = the reference: one
 * register-staged kernel with one key group at every size.  The DMA forms permute a tile's keys among the score rows (the same products
 * summed in another order inside a matrix-core k group) and the four-group form sums the key tiles in four interleaved partial states:
 * default and reference agree to fp32 round-off, 3-4e-3 of the mel range after the 10 Euler steps, NOT bit for bit.  For the same reason
 * a batch that crosses a block-count switch differs from the same utterances run alone by that margin. */
int cv2_flow_debug_attn_dma(int32_t on);
/* Test hook: 1 = cv2_flow_inference captures the launches of a call into a hipGraph at the second use of a shape (token / prompt lengths, flags)
 * and replays it from then on (bit-identical results; CV2_FLOW_GRAPH=1), 0 = always the launches, -1 = the environment (default off: measured
 * 0.4 ms slower per configs[1] utterance, profiles/r6_flow_graph_ab.txt). */
int cv2_flow_debug_graph(int32_t on);

/* The estimator alone behind the reference's TensorRT seam (flow_matching.py:125-150): six contiguous device
 * tensors x(2,80,T) mask(2,1,T) mu(2,80,T) t(2,) spks(2,80) cond(2,80,T), result written in place into x. */
int cv2_flow_estimator(cv2_flow* h, float* x, const float* mask, const float* mu, const float* t, const float* spks,
                       const float* cond, int32_t T, int32_t streaming, void* stream);
/* The encoder alone (UpsampleConformerEncoder.forward): xs fp32 [T][512] embedded tokens (+ optional context [3][512]),
 * out fp32 [2T][512]. */
int cv2_flow_encoder(cv2_flow* h, const float* xs, int32_t T, const float* context, int32_t streaming, float* out, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Stage 3 — HiFT vocoder (replaces HiFTGenerator.inference, cosyvoice/hifigan/generator.py:570-582, and decode :520-552,
 * _stft/_istft :504-518, ResBlock :94-101, SourceModuleHnNSF2 :375-389, SineGen2 :256-339, ConvRNNF0Predictor
 * f0_predictor.py:55-58).  fp32 storage and accumulation throughout.
 *
 * Conv weights (weight-norm already folded, w = g v / ||v||) are fp32 in the MFMA 32x32x2 B-operand order
 * [tap][c_in/2][c_out/32][64 lanes], lane = (c_in & 1) * 32 + (c_out & 31), both channel counts zero-padded to 64.
 * A ConvTranspose1d(stride u, kernel k, padding p) is stored as its polyphase Conv1d with u*C_out output channels
 * (index r*C_out + c_out) over 3 taps: W'[r*C_out + c_out][c_in][j] = W[c_in][c_out][r + p + u (1 - j)] where that
 * index lies in [0, k), else 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cv2_hift cv2_hift;
typedef struct {
    const float* w; const float* b;     /* packed weight, bias [cout_pad] */
    int32_t cin, cout, cin_pad, cout_pad, taps, dil, pad_left;
    const uint16_t* w3;                 /* optional: the same weight as three bf16 planes (w = w0 + w1 + w2, each the bf16 rounding of the
                                           remainder) in the MFMA 32x32x16 B-operand order [tap][c_in/16][c_out/32][plane][64 lanes][8],
                                           lane = ((c_in % 16) / 8) * 32 + (c_out & 31), element = c_in % 8.  When given, the convolution runs
                                           on the bf16 matrix cores with six products per term (fp32-equivalent accuracy, csrc/hift.hip k_conv6);
                                           NULL: fp32 matrix cores (exact fp32 FMA chains; kept for the f0 predictor, whose output is integrated
                                           into a 1e5-rad phase) */
} cv2_conv;
typedef struct {                          /* ResBlock: convs1 (dilated), convs2, Snake alphas */
    cv2_conv c1[3], c2[3];
    const float* a1[3]; const float* a2[3];
} cv2_resblock;
typedef struct {
    cv2_conv f0_conv[5];                  /* f0_predictor.condnet.{0,2,4,6,8} */
    const float* f0_w; const float* f0_b; /* f0_predictor.classifier [512], [1] */
    const float* src_w; const float* src_b; /* m_source.l_linear [9], [1] */
    cv2_conv conv_pre;
    cv2_conv ups[3];
    const float* sd_w[3]; const float* sd_b[3];  /* source_downs weights re-ordered [k][18][C] (the scalar kernel; used when sd_conv[i].w3 is NULL) */
    cv2_conv sd_conv[3];                  /* source_downs.{0,1,2} (generator.py:468-479) as 1-tap convolutions over flat windows of the [F][18] STFT rows:
                                             cin = 18 k with input index j * 18 + c for tap j, channel c; taps = 1; w3 given -> they run on the matrix cores */
    cv2_resblock src_rb[3];
    cv2_resblock rb[9];
    cv2_conv conv_post;
} cv2_hift_weights;
typedef struct { int32_t max_frames; int32_t lanes; } cv2_hift_dims;   /* longest mel in frames; lanes > 1: workspace copies for cv2_hift_inference_batch */

size_t cv2_hift_workspace_bytes(const cv2_hift_dims* d);
int cv2_hift_create(const cv2_hift_dims* d, const cv2_hift_weights* w, void* workspace, size_t workspace_bytes, cv2_hift** out);
int cv2_hift_destroy(cv2_hift* h);
/* Test hook: pair / xcd_split = 1 / 0 runs the vocoder with / without the fused ResBlock pairs of the 64- and 128-channel stages (one launch
 * per (dilated conv, conv) pair, the intermediate kept in LDS) and with / without the per-layer split of the convolution grids over the XCDs;
 * -1 = the default.  All four combinations produce the same waveform bit for bit.  Process-wide; calls of <= 160 frames replay graphs
 * captured under the mode of their first call. */
int cv2_hift_debug_modes(int32_t pair, int32_t xcd_split);
/* Test hook: how the convolutions with plane weights multiply.  2 = two bf16 planes per operand, three products (~2^-15 of a term; the
 * default since round 6), 0 = three planes, six products (fp32-equivalent; CV2_HIFT_PLANES=3), 1 = the fp32 matrix-core kernel everywhere
 * (CV2_HIFT_FP32=1), -1 = what the environment says.  Process-wide; graphs as for cv2_hift_debug_modes. */
int cv2_hift_debug_precision(int32_t mode);
/* Test hook: the f0 track [T] (Hz; ConvRNNF0Predictor.forward, f0_predictor.py:55-58) of the engine's last cv2_hift_inference call. */
int cv2_hift_debug_f0(cv2_hift* h, float* out, int32_t T, void* stream);
/* mel fp32 [80][T] (channel-major, the reference's speech_feat[0]); cache_source fp32 [n_cache] or NULL;
 * noise: fp32 [480 T][9] standard normals injected in place of the reference's randn_like (generator.py:334), or NULL
 * to draw them on the device from Philox(seed); wav fp32 [480 T]; source fp32 [480 T]. */
int cv2_hift_inference(cv2_hift* h, const float* mel, int32_t T, const float* cache_source, int32_t n_cache,
                       const float* noise, uint64_t seed, float* wav, float* source, void* stream);
/* n <= lanes chunks of ONE shape (T <= 160 frames, n_cache cached source samples each) as one set of launches (gridDim.z = n): the
 * chunks of a streaming round (cli/model.py:351-381 x the concurrent streams).  Arrays of n device pointers / seeds on the host; the
 * results equal n cv2_hift_inference calls with the same seeds. */
int cv2_hift_inference_batch(cv2_hift* h, int32_t n, const float* const* mel, int32_t T, const float* const* cache_source, int32_t n_cache,
                             const uint64_t* seeds, float* const* wav, float* const* source, void* stream);

/* fade_in_out (cosyvoice/utils/common.py:142-150): new[:w] = new[:w] * win[:w] + old[-w:] * win[w:], in place on `fade_in`;
 * win fp32 [2w] (np.hamming(2w)), old_tail points at the last w samples of the previous chunk. */
int cv2_fade_in_out(float* fade_in, const float* old_tail, const float* window, int32_t w, void* stream);
/* cli/model.py:328-330 (speed != 1, non-streaming): out[r][j] = linear interpolation of in[r][.] at (j + 0.5) n_in / n_out - 0.5
 * (torch.nn.functional.interpolate(mode='linear'), align_corners False); in [rows][n_in], out [rows][n_out], fp32 device. */
int cv2_interp_linear(const float* in, float* out, int32_t rows, int32_t n_in, int32_t n_out, void* stream);

/* Streaming calls with speed != 1 (an extension: the reference asserts, cli/model.py:328): a time-stretch of the mel defined on the GLOBAL
 * frame index of the stream, so that chunk boundaries cannot change a value.  m[0 .. N) are the frames a streaming call hands to the vocoder
 * stage, in order; with r = (float)speed output frame j is w0 m[i0] + w1 m[i1], x = max(0, fma(r, j + 0.5, -0.5)) in fp32 from the global j (one
 * rounding), i0 = floor(x), i1 = min(i0 + 1, n_final - 1), w1 = x - i0, w0 = 1 - w1.  One call emits the
 * frames j0 .. j0 + n_emit - 1 of one stream; which frames can be emitted and which source frames stay is planned on the host
 * (cv2amd/stretch.py evaluates the same fp32 expression).  The source frames first .. n_available - 1 are given as two pieces: `tail`
 * (n_tail frames from global index `first` on, retained from earlier chunks) and `fresh` (the n_available - first - n_tail new frames);
 * both [rows][ld] fp32, time contiguous.  Frame j lands at dst[row * ld_dst + dst_col + (j - j0)]: straight behind the cached mel frames of
 * the vocoder's input.  n_final: -1 while more frames will come (then every i0 + 1 <= n_available - 1 is required), else = n_available.
 * 0.25 <= r <= 4; j0 + n_emit <= 2^23.  Adding these entry points changed no struct and no signature: CV2_ABI_VERSION stays. */
typedef struct {
    const float* tail; const float* fresh; float* dst;
    int32_t ld_tail, ld_new, ld_dst, dst_col;
    int32_t first, n_tail, n_avail;
    int32_t j0, n_emit, n_final;
    float r;
    int32_t reserved;
} cv2_stretch_args;                                                  /* 72 bytes */
int cv2_mel_stretch(const cv2_stretch_args* a, int32_t rows, void* stream);       /* a: host */
/* n streams as ONE launch (gridDim.z = n): `args` are the n records on the host (checked here), `table_dev` the same n records in device
 * memory, uploaded by the caller ahead of this call on `stream` -- the kernel reads its stream's record from there. */
int cv2_mel_stretch_batch(const cv2_stretch_args* args, const cv2_stretch_args* table_dev, int32_t n, int32_t rows, void* stream);

/* Output rate and sample format of a call (an extension: the reference hands back float32 at 24 kHz and nothing else): the waveform resampled
 * to a target rate R and / or converted to int16 PCM on the device, ahead of the device-to-host copy, chunk-invariant when streaming.
 * s[0 .. N) are the 24 kHz samples a call yields, in order (a streaming call: the concatenation of its chunks after cross-fade and cache
 * trim).  g = gcd(24000, R), down = 24000 / g, up = R / g; K[up][klen] and width are torchaudio's sinc_interp_hann table for 24000 -> R
 * (lowpass width 6, rolloff 0.99, fp64 rounded once to fp32: cv2amd.prompt._sinc_kernel, the table cv2_resample takes).  Output sample
 * o = i up + p, 0 <= p < up, is
 *     y[o] = sum over j = 0 .. klen - 1 with 0 <= q < N of K[p][j] s[q],   q = i down - width + j,
 * ONE fp32 fmaf chain in ascending j from 0.f; taps outside [0, N) are skipped, not multiplied by zero (k_resample's order: a stream equals
 * cv2_resample of the whole signal bit for bit, whatever the chunking).  The call emits ceil(N up / down) samples in all.  Before the final
 * chunk o goes out as soon as i down - width + klen - 1 <= n_available - 1; the final chunk emits the rest.  Retained per call: the source
 * samples from max(0, i_next down - width) on (fewer than klen + down).  All index arithmetic is integer; cv2amd/outrate.py plans it.
 * One record = one call's chunk: the source samples first .. n_available - 1 as two pieces, `tail` (n_tail samples from global index `first`
 * on) and `fresh` (the n_available - first - n_tail new ones), both fp32 device; the outputs o0 .. o0 + n_emit - 1 go to dst[0 .. n_emit),
 * float (CV2_OUT_F32) or int16 (CV2_OUT_PCM16: trunc_toward_zero(y * 32768) saturated to [-32768, 32767], NaN -> 0; for in-range values
 * the servers' (x * 2**15).astype(int16)).  dst is aligned to its element only; dst_cap = elements it can take.  n_final: -1 while more
 * samples will come, else = n_available.  kernel = NULL with up = down = klen = 1, width = 0: no filter (R = 24000), the samples pass through
 * exactly.  Records of one batch may differ in rate and format.  Adding these entry points changed no struct and no signature:
 * CV2_ABI_VERSION stays. */
#define CV2_OUT_F32 0
#define CV2_OUT_PCM16 1
typedef struct {
    const float* tail; const float* fresh; void* dst; const float* kernel;
    int32_t first, n_tail, n_avail, n_final;
    int32_t o0, n_emit;
    int32_t up, down, klen, width;
    int32_t format, dst_cap;
} cv2_out_args;                                                      /* 80 bytes */
int cv2_out_resample(const cv2_out_args* a, void* stream);                        /* a: host */
/* n calls as ONE launch (gridDim.z = n): `args` are the n records on the host (checked here), `table_dev` the same n records in device
 * memory, uploaded by the caller ahead of this call on `stream`. */
int cv2_out_resample_batch(const cv2_out_args* args, const cv2_out_args* table_dev, int32_t n, void* stream);

/* Joined calls (an extension: the reference yields the segments of a split text one by one, cli/cosyvoice.py:181-210): the 24 kHz waveforms
 * s_0 .. s_{k-1} (lengths n_i, fp32 device, aligned to 4 bytes only) of ONE call's text segments written into one waveform on the device.
 *
 * cv2_wave_bounds -- the kept range [a_i, b_i) of every segment when interior silences are trimmed, all k segments in one call:
 *   frames of 240 samples without overlap, frame f = [240 f, min(240 f + 240, n_i));  peak_f = max |s_i[q]| over the frame, a NaN sample
 *   counting as 0;  P_i = max_f peak_f;  thr_i = P_i * g, ONE fp32 product (g = float32(10 ** (-trim_db / 20)), rounded once on the host);
 *   frame f is loud iff P_i > 0 and peak_f >= thr_i.  With f_lo / f_hi the first / last loud frame and keep = 480:
 *       a_i = max(0, 240 f_lo - keep) for i > 0, else 0;      b_i = min(n_i, 240 (f_hi + 1) + keep) for i < k - 1, else n_i;
 *   a segment with P_i == 0 keeps a_i = 0, b_i = n_i.  Only interior edges are trimmed.  Every quantity is a maximum or the one rounded
 *   product: integer atomics (atomicMin / atomicMax, order-independent; P_i through the bit pattern of a non-negative float) and no float
 *   atomic, so a host restatement gives the same integers.  bounds_dev [k][2] receives (a_i, b_i), peaks_dev [k] receives P_i; both are
 *   written whole (no need to clear them).  Three stream operations (a clear of peaks_dev, the peaks, the loud frames), one entry-point call.
 * cv2_wave_join -- the pieces s_i[src_off .. src_off + m) written to dst[dst_off .. dst_off + m), pieces in ascending dst_off, one launch:
 *   with CV2_WAVE_FADE_IN the first F samples of a piece are multiplied by w[t], with CV2_WAVE_FADE_OUT its last F samples by w[F - 1 - t]
 *   (t counted from the start of the faded range; w = fade_table_dev [F], 0.5 - 0.5 cos(pi (t + 0.5) / F) in fp64 rounded once to fp32 on
 *   the host): ONE fp32 multiply per sample; every other sample of a piece is copied bit for bit; every sample of dst[0 .. n_dst) that no
 *   piece covers is written as +0.0f (dst need not be cleared).  dst is aligned to 4 bytes only.
 * Both take their records twice, as cv2_out_resample_batch does: on the host (checked here: k in 1 .. CV2_WAVE_MAX_PIECES; segment
 * lengths n in 1 .. 2^30 for the bounds, 0 <= m <= n_src <= 2^30 for a piece -- an empty piece writes nothing --; 0 < g <= 1; pieces
 * ordered, not overlapping, inside n_dst and inside their sources; F >= 0; a fade flag needs m >= 2 F; -1 and cv2_last_error otherwise,
 * nothing launched) and in device memory, uploaded by the caller ahead of the call on `stream`.
 * Adding these entry points changed no struct and no signature: CV2_ABI_VERSION stays. */
#define CV2_WAVE_MAX_PIECES 256
#define CV2_WAVE_FADE_IN 1
#define CV2_WAVE_FADE_OUT 2
typedef struct {
    const float* src; int32_t n; int32_t reserved;
} cv2_wave_seg;                                                      /* 16 bytes */
typedef struct {
    const float* src; int32_t n_src, src_off, m, dst_off, fade, reserved;
} cv2_wave_piece;                                                    /* 32 bytes */
int cv2_wave_bounds(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t k, float g, int32_t* bounds_dev, float* peaks_dev,
                    void* stream);
int cv2_wave_join(const cv2_wave_piece* pieces, const cv2_wave_piece* pieces_dev, int32_t k, const float* fade_table_dev, int32_t F,
                  float* dst, int32_t n_dst, void* stream);

/* Continuous calls (an extension): the 24 kHz chunks of ONE call's text segments, as the streaming path produces them, written into one
 * stream chunk by chunk -- what cv2_wave_bounds / cv2_wave_join do for whole waveforms, with a CAUSAL gate in place of the trim (the trim's
 * threshold is relative to the segment's peak, known at its end only).  s_i[0 .. n_i) is segment i of k, delivered in chunks.
 *
 * cv2_wave_gate_chunk -- frames f0 .. f1 - 1 of the current segment (240 samples without overlap; the short last frame only once the
 *   segment has ended): peak_f as for cv2_wave_bounds; C_i = the maximum of |s| over every sample of the segments before i (C_0 = 0);
 *   R_i(f) = max(C_i, peak_0, .., peak_f); frame f is loud iff R_i(f) > 0 and peak_f >= R_i(f) * g, ONE fp32 product.  Only maxima and that
 *   product: a host restatement gives the same integers, whatever the chunk boundaries.  seg_start = 1 on a segment's first call (C takes the
 *   running maximum, first / last loud frame are cleared).  The segment's samples from held_start on are [held (n_held) | chunk (n_new)];
 *   240 f0 >= held_start.  record_dev [4] receives (first loud frame of the segment so far or -1, last loud frame or -1, f1, the bits of R);
 *   the same values stay in *state_dev.  One block; f0 == f1 is allowed.
 * cv2_wave_emit_chunk -- one launch writes dst[0 .. e1 - e0 + n_zero) = the segment's samples e0 .. e1 - 1 followed by n_zero samples +0.0f,
 *   and held_dst[0 ..) = the samples from keep_from on (what stays held, compacted; held_dst is another buffer than held).  A sample q of
 *   [fade_in_at, fade_in_at + F) is multiplied by w[q - fade_in_at], one of [fade_out_end - F, fade_out_end) by w[fade_out_end - 1 - q]
 *   (w, F as for cv2_wave_join; -1: no such fade): ONE fp32 multiply; every other sample is copied bit for bit.  dst and held_dst are
 *   aligned to 4 bytes only.  Checked here (-1 and cv2_last_error otherwise, nothing launched): held_start <= e0 <= e1 <= keep_from <=
 *   held_start + n_held + n_new <= 2^30; 0 <= F <= 120; a tail fade ends at e1 and lies inside the emission, the fades do not overlap;
 *   what stays fits held_cap; no two of dst, held_dst and the sources overlap.
 * *state_dev (32 bytes, zeroed by the caller when the call starts) is written by these kernels only.  `a` is read on the host.
 * Adding these entry points changed no existing struct and no signature: CV2_ABI_VERSION stays. */
typedef struct {
    uint32_t r_bits, c_bits;                     /* bits of the running maximum R (R includes C_i: the gate reads r_bits only) and of C_i (kept for inspection) */
    int32_t frames, f_lo, f_hi;                  /* frames of the segment analysed; its first / last loud frame so far, -1: none */
    int32_t n_held, held_start, reserved;        /* the held samples: how many, and the segment position of the first */
} cv2_wave_state;                                                    /* 32 bytes */
typedef struct {
    const float* held; const float* chunk; const float* fade_table; float* dst; float* held_dst;
    int32_t held_start, n_held, n_new, e0, e1, fade_in_at, fade_out_end, F, n_zero, keep_from, held_cap, reserved;
} cv2_wave_emit;                                                     /* 88 bytes */
int cv2_wave_gate_chunk(cv2_wave_state* state_dev, const float* held, int32_t held_start, int32_t n_held, const float* chunk, int32_t n_new,
                        int32_t f0, int32_t f1, int32_t seg_start, float g, int32_t* record_dev, void* stream);
int cv2_wave_emit_chunk(cv2_wave_state* state_dev, const cv2_wave_emit* a, void* stream);

/* Output level of a call (an extension: the reference hands back whatever level its prompt gives it): a fixed gain, an optional scaling of the
 * call's peak to a target, and a look-ahead limiter under a ceiling, on the device, AHEAD of cv2_out_resample, chunk-invariant when streaming.
 * s[0 .. N) are the 24 kHz samples that reach the output stage (after fade and trim; the joined waveform; the one signal of a continuous
 * call).  All fp32.  G = float32(10 ** (gain_db / 20)), c = float32(10 ** (ceiling_db / 20)), T = float32(10 ** (peak_db / 20)), each computed
 * in fp64 on the host and rounded once; L = look-ahead in samples, 24 .. 240; w[j] = h_j / sum h, h_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / (L + 1)),
 * j = 0 .. L (fp64, rounded once).  Ge = G, or with a peak target P = max |s[n]| (NaN counts as 0): Ge = fl(G * fl(T / P)) when P > 0.
 *     x[n] = fl(Ge s[n]);   a[n] = |x[n]|, NaN counts as 0;   r[n] = a[n] > c ? fl(c / a[n]) : 1;   d[n] = a[n] > c ? fl(1 - r[n]) : 0
 *     D[n] = max d[k], k = n .. min(n + L, N - 1)
 *     acc[n] = sum over j = 0 .. L with n - j >= 0 of w[j] D[n - j]       ONE fp32 fmaf chain in ascending j from 0.f
 *     g[n] = max(0, min(fl(1 - acc[n]), r[n]));   y[n] = clamp(fl(g[n] x[n]), -c, c);   a NaN x[n] gives +0, an infinite one +-c
 * |y| <= c always; where no sample within +-L of n is over the ceiling acc is exactly 0 and y[n] = x[n] (= s[n] bit for bit when Ge = 1);
 * N samples in, N out, no index delay.  Before the final chunk sample n goes out as soon as n + L <= n_available - 1; the final chunk emits
 * the rest.  Retained per call: the source samples from max(0, n_next - L) on (at most 2 L).  cv2amd/level.py plans the integers.
 * One record = one call's chunk: the source samples first .. n_avail - 1 as two pieces, `tail` (n_tail samples from global index `first` on)
 * and `fresh` (the n_avail - first - n_tail new ones), both fp32 device, aligned to 4 bytes only; the outputs n0 .. n0 + n_emit - 1 go to
 * dst[0 .. n_emit) (fp32 device, aligned to 4 bytes only; dst_cap = samples it can take).  n_final: -1 while more samples will come, else
 * = n_avail.  weights = w (device, L + 1 floats).  peak = NULL: Ge is the gain applied; else a device float holding P (cv2_level_peak_batch
 * ahead of this call on the same stream: the kernel reads it, the host never does), Ge holds G, T the target, n_final >= 0.  Checked here
 * (-1 and cv2_last_error otherwise, nothing launched): L in 24 .. 240; 0 < c <= 1; 0 < Ge <= 16; 0 < T <= c; the counts; max(0, n0 - L) >=
 * first; n0 + n_emit - 1 + L <= n_avail - 1 before the final chunk, n0 + n_emit <= n_final in it; n_emit <= dst_cap.  Records of one batch
 * may differ in every field.
 * cv2_level_peak_batch -- peaks_dev[i] = max |s_i[q]| (NaN counts as 0) of n signals (cv2_wave_seg records, on the host and in device memory
 * as for cv2_wave_bounds; a length of 0 gives 0): a clear of peaks_dev and one launch, an integer atomicMax on the bit pattern per block.
 * Adding these entry points changed no existing struct and no signature: CV2_ABI_VERSION stays. */
typedef struct {
    const float* tail; const float* fresh; float* dst; const float* weights; const float* peak;
    int32_t first, n_tail, n_avail, n_final;
    int32_t n0, n_emit, L, dst_cap;
    float Ge, c, T; int32_t reserved;
} cv2_level_args;                                                    /* 88 bytes */
int cv2_level_chunk(const cv2_level_args* a, void* stream);                       /* a: host */
/* n calls as ONE launch (gridDim.z = n): `args` are the n records on the host (checked here), `table_dev` the same n records in device
 * memory, uploaded by the caller ahead of this call on `stream`. */
int cv2_level_chunk_batch(const cv2_level_args* args, const cv2_level_args* table_dev, int32_t n, void* stream);
int cv2_level_peak_batch(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t n, float* peaks_dev, void* stream);

/* Integrated loudness of a call (an extension; ITU-R BS.1770-4 at fs = 24000), measured on the device so that cv2_level_chunk can scale a call
 * to a loudness target: csrc/loudness.hip.  s[0 .. N) are the 24 kHz fp32 samples that enter the level stage; a non-finite sample counts as 0.
 *   K-weighting: two biquads in cascade (transposed direct form II, fp32), the shelf, then the high-pass; coefficients from the analog
 *     prototype that reproduces the BS.1770 table at 48 kHz, in float64 on the host, rounded once; K = tan(pi f0 / fs), a0 = 1 + K / Q + K^2:
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20), Vb = Vh^0.4996667741545416,
 *                b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *   Blocks: hop 2400 samples; block j = y[2400 j .. 2400 j + 9600), j = 0 .. J - 1, J = floor((N - 9600) / 2400) + 1 when N >= 9600, else 0;
 *     z_j = mean y^2 over block j, l_j = -0.691 + 10 log10 z_j.
 *   Gates: A = {j : l_j > -70}; Gamma = -0.691 + 10 log10 mean_A z_j - 10; B = {j in A : l_j > Gamma}; z = mean_B z_j; Lk = -0.691 + 10 log10 z.
 *   No block or A empty: Lk = -inf, R = 0.  Else R = sqrt(z), with a target T > 0 clamped to [T / g_max, T g_max], g_max = float32(10^(24/20)).
 * cv2_loudness_batch -- n signals (cv2_wave_seg records on the host, checked here, and the same records in device memory, as for
 * cv2_level_peak_batch; sources aligned to 4 bytes only), all in one enqueue on `stream` (four launches; no allocation, no synchronisation,
 * no atomics): R_dev[i] and lufs_dev[i] receive R and Lk of signal i.  targets / targets_dev: T per signal on the host and in device memory
 * (0 <= T <= 1, 0: R is not clamped), or both NULL.  filter_dev: 24 floats in device memory -- shelf b0 b1 b2 a1 a2, high-pass a1 a2, 0, then
 * M = A^2400 row-major, A the 4 x 4 transition matrix of the cascade's state (s1, s2, t1, t2) for a zero input (cv2amd/loudness.py builds it
 * in float64).  ws: the caller's scratch for the hop states and hop energies, 16-byte aligned, at least the size that
 * cv2_loudness_workspace_bytes gives for the same records; its contents need not be kept or cleared.  The result is a function of each
 * signal's samples alone: bit-equal whatever shares the launch, wherever the buffers lie.  -1 and cv2_last_error, nothing launched, for a
 * length outside 0 .. 2^30, a missing table or source, a target out of range or a workspace that is too small.
 * Adding these entry points changed no existing struct and no signature: CV2_ABI_VERSION stays. */
int cv2_loudness_workspace_bytes(const cv2_wave_seg* segs, int32_t n, size_t* bytes);
int cv2_loudness_batch(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t n, const float* targets, const float* targets_dev,
                       const float* filter_dev, float* R_dev, float* lufs_dev, void* ws, size_t ws_bytes, void* stream);

/* =====================================================================================================================
 * Prompt features (the extractor that feeds this path): replaces the reference's
 *   feat_extractor = matcha.utils.audio.mel_spectrogram(n_fft 1920, num_mels 80, sampling_rate 24000, hop_size 480, win_size 1920,
 *                    fmin 0, fmax 8000, center False)          conf/cosyvoice2.yaml:152-160, third_party/Matcha-TTS/matcha/utils/audio.py:45-82
 *   torchaudio.transforms.Resample(16000, 24000)               cli/frontend.py:497 (torchaudio 2.3.1, functional.py _apply_sinc_resample_kernel)
 * Table-driven: the host computes window, twiddles, mel filterbank and the polyphase kernel (cv2amd/prompt.py), all DEVICE pointers.
 * cv2_melspec: wav fp32 [n]; out fp32 [n_frames][n_mels] time-major (= prompt_speech_feat[0]); reflect padding (n_fft - hop) / 2 on both
 *   sides, frames of n_fft at stride hop, |DFT| = sqrt(re^2 + im^2 + 1e-9), out = log(max(mel_fb @ |DFT|, clamp_min));
 *   n_frames = 1 + (n + (n_fft - hop) - n_fft) / hop.
 * cv2_resample: out[i * up + p] = sum_j kernel[p][j] * xpad[i * down + j], xpad = zeros(pad_left) ++ in ++ zeros; n_out <= ceil(n_in * up / down). */
typedef struct {
    int32_t n_fft, hop, n_mels, n_bins;          /* n_bins = n_fft / 2 + 1 */
    const double* window;                        /* [n_fft] fp64 */
    const double* twiddle;                       /* [n_fft][2] fp64: cos, sin of 2 pi j / n_fft */
    const float* mel_fb;                         /* [n_mels][n_bins] */
    const int32_t* fb_lo; const int32_t* fb_hi;  /* [n_mels]: filter m is zero outside bins [fb_lo[m], fb_hi[m]) */
    float clamp_min;
} cv2_melspec_cfg;
int cv2_melspec(const cv2_melspec_cfg* cfg, const float* wav, int64_t n, float* out, int32_t n_frames, void* stream);
int cv2_resample(const float* in, int64_t n_in, const float* kernel, int32_t up, int32_t down, int32_t klen, int32_t pad_left,
                 float* out, int64_t n_out, void* stream);

/* The two feature extractors in front of the ONNX prompt models (cosyvoice/cli/frontend.py:262-283; third-party algorithms):
 *   whisper.log_mel_spectrogram(speech, n_mels=128) -> speech_tokenizer_v2.onnx   (frontend.py:264): center = 1, win = n_fft = 400, hop 160,
 *       periodic Hann window, |X|^2 of every frame but the last, Slaney filters [128][201], log10(max(., 1e-10));
 *       cv2_whisper_post: max(x, max(x) - 8), (x + 4) / 4, transposed to [n_mels][frames] (the layout the ONNX graph takes)
 *   torchaudio.compliance.kaldi.fbank(speech, num_mel_bins=80, dither=0, sample_frequency=16000) -> campplus.onnx (frontend.py:277):
 *       center = 0 (snip_edges), win 400, n_fft 512 (zero padded), hop 160, remove_dc = 1, preemph 0.97, povey window, |X|^2, kaldi mel
 *       banks [80][257] (20 Hz .. Nyquist), ln(max(., FLT_EPSILON)); cv2_sub_col_mean: feat - feat.mean(dim=0) (frontend.py:278)
 * cv2_framefeat: wav fp32 [n]; out fp32 [n_frames][n_mels]; n_frames = n / hop (center) or 1 + (n - win) / hop (snip_edges).
 * Tables are DEVICE pointers computed by the host (cv2amd/prompt.py). */
typedef struct {
    int32_t n_fft, win, hop, n_bins, n_mels;     /* win <= n_fft: the windowed frame is zero-padded to the DFT length */
    const double* window;                        /* [win] fp64 */
    const double* twiddle;                       /* [n_fft][2] fp64: cos, sin of 2 pi j / n_fft */
    const float* mel_fb;                         /* [n_mels][n_bins] */
    const int32_t* fb_lo; const int32_t* fb_hi;  /* [n_mels]: filter m is zero outside bins [fb_lo[m], fb_hi[m]) */
    int32_t center, remove_dc;
    float preemph;
    int32_t log10;                               /* 1: log10, 0: natural log */
    float floor;                                 /* clamp before the log */
} cv2_framefeat_cfg;
int cv2_framefeat(const cv2_framefeat_cfg* cfg, const float* wav, int64_t n, float* out, int32_t n_frames, void* stream);
int cv2_whisper_post(const float* in, float* out, int32_t n_frames, int32_t n_mels, void* stream);
int cv2_sub_col_mean(float* x, int32_t n_rows, int32_t n_cols, void* stream);

/* Test hooks: the element-wise functions exactly as the kernels evaluate them (fast-math exp / sin / reciprocal), so that their
 * error against libm can be swept over the input ranges of the real checkpoint (tests/test_math_gpu.py).
 *   act: 1 exact-erf GELU (diffusers GELU, matcha transformer.py FeedForward), 2 SiLU, 3 Mish, 4 leaky ReLU (slope)
 *   pre: 1 Snake x + sin^2(alpha x) / (alpha + 1e-9) (hifigan/generator.py ResBlock activations), 2 leaky ReLU (slope) */
int cv2_dbg_act(const float* x, float* out, int64_t n, int32_t act, float slope, void* stream);
int cv2_dbg_pre(const float* x, float* out, int64_t n, int32_t pre, float alpha, float slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif
