/* mmrag.h -- C-ABI of the MI355X-native embed-and-retrieve engine (libmmrag.so).
 *
 * Drop-in boundary for the hot path of someone-in-somewhere/multimodal_rag
 * (app/utils/embedder.py).  The reference has no FFI of its own: its arithmetic lives in
 * two third-party engines that embedder.py calls through Python.  Each entry point below
 * replaces one of those engine calls; INTEGRATION.md shows the ctypes stub a maintainer
 * of the reference would add at the cited call site.
 *
 * Conventions
 *   - plain pointers and sizes only; every `dev` pointer is HIP device memory owned by the
 *     caller (in this repo: torch tensors' data_ptr()); nothing is retained past return;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is
 *     enqueued on it and the call returns without synchronising;
 *   - return value: 0 = ok, otherwise an MMRAG_E* code; mmrag_last_error() gives the
 *     message for the calling thread.  No entry point aborts or throws;
 *   - re-entrant: no global mutable scratch; callers pass a workspace sized by the matching
 *     *_workspace_bytes() query (embedder.py:368/595 call the engines from thread-pool
 *     workers, SURVEY.md section 8b "Threading").
 *
 * There is NO CPU fallback behind these symbols: without a gfx950 device they fail.
 */
#ifndef MMRAG_H
#define MMRAG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMRAG_OK 0
#define MMRAG_EINVAL 1   /* bad argument (shape, alignment, dtype, k) */
#define MMRAG_EWORKSPACE 2 /* workspace too small */
#define MMRAG_EHIP 3     /* a HIP runtime call failed */
#define MMRAG_EUNSUPPORTED 4

/* storage dtype of vectors / weights / activations */
#define MMRAG_F32 0
#define MMRAG_F16 1
#define MMRAG_BF16 2
/* FP8 collections (gfx950 is OCP, not fnuz).  A stored element is the OCP E4M3 code of x * 256, rounded to nearest
 * even from float32: subnormals kept, magnitudes above 448 saturate to 448, NaN stores +0.  Rows and queries share
 * the constant scale 2^8, so a score is acc * 2^-16 (an exact scaling of the float32 accumulator).  Rows are padded
 * to 128 elements (one 128-byte K-slab), pad columns are code 0x00.  Accepted by mmrag_padded_dim, append / gather /
 * fetch rows, mmrag_cosine_topk(_lists) and mmrag_cosine_topk_deep (q and corpus both dtype 3); nowhere else. */
#define MMRAG_F8E4M3 3

#define MMRAG_MAX_K 20 /* api.py:163  top_k: int = Field(5, ge=1, le=20) */

int mmrag_abi_version(void);
const char *mmrag_last_error(void);

/* Leading dimension (in elements) the corpus / query matrices must be padded to for `d`
 * logical columns of `dtype`: rows are streamed in 128-byte K-slabs.  Pad columns are 0. */
int64_t mmrag_padded_dim(int d, int dtype);

/* ---------------------------------------------------------------------------------------
 * Retrieve.  Replaces chromadb's  collection.query(query_embeddings=[v], n_results=k, ...)
 * reference call site: app/utils/embedder.py:595-601 (and :900-905), result flattening
 * :604-609.  Exact batched inner-product k-NN (rows are unit-norm => cosine), fused
 * Q x corpus^T MFMA GEMM + per-query top-k selection; the [B, n] score matrix never
 * reaches HBM.
 *
 *   q          dev [B, ld]      queries, dtype `dtype`, pad columns zero
 *   corpus     dev [n, ld]      this shard's rows, same dtype / ld, pad columns zero
 *   ld         = mmrag_padded_dim(d, dtype) or any larger multiple of it
 *   k          1..MMRAG_MAX_K
 *   row_offset added to local row numbers => global row ids (shard base)
 *   alive_bits dev, optional (NULL = all alive): bit r%32 of word r/32 set <=> row r may be
 *              returned (delete_document tombstones embedder.py:619-656, `where` filters :599)
 *   out_scores dev [B, k] float32, descending; ties -> lower row first
 *   out_rows   dev [B, k] int64 global rows; (-inf, -1) padding when fewer than k live rows
 *   workspace  dev, >= mmrag_cosine_topk_workspace_bytes(B, n, k) bytes, 16-byte aligned
 * ------------------------------------------------------------------------------------- */
size_t mmrag_cosine_topk_workspace_bytes(int B, int64_t n, int k);

int mmrag_cosine_topk(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                      int dtype, int k, int64_t row_offset, const uint32_t *alive_bits,
                      float *out_scores, int64_t *out_rows, void *workspace,
                      size_t workspace_bytes, void *stream);

/* The same search as two stream-ordered phases, so a caller can time, overlap or graph-capture
 * them separately: phase 1 = the fused GEMM + per-lane selection kernel (reads the corpus once,
 * leaves candidate lists in `workspace`); phase 2 = the small per-query merge of those lists.
 * mmrag_cosine_topk(...) == lists(...) then select(...) with the same B, n, k, workspace. */
int mmrag_cosine_topk_lists(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                            int dtype, int k, const uint32_t *alive_bits, void *workspace,
                            size_t workspace_bytes, void *stream);
int mmrag_cosine_topk_select(int B, int64_t n, int k, int64_t row_offset, const void *workspace,
                             float *out_scores, int64_t *out_rows, void *stream);

/* Deep exact top-k: the same search for any k in 1..MMRAG_MAX_K_DEEP (Chroma's n_results has no cap of 20).
 * Same arguments, layout, ordering, padding and error codes as mmrag_cosine_topk; scores are bit-identical to
 * it (the same GEMM), and its first 20 results are those of mmrag_cosine_topk(k = 20).  A bound from a strided
 * sample, a threshold-filter scan into per-query candidate buffers and a per-query radix select, all
 * stream-ordered on `stream`; a query whose survivors overflow its buffer is re-run alone, exactly.
 * It SYNCHRONISES `stream` once (to read the per-query survivor counts; not at all when n is small enough that
 * nothing can overflow), so it cannot be captured into a graph.
 *   workspace  dev, >= mmrag_cosine_topk_deep_workspace_bytes(B, n, k) bytes, 16-byte aligned
 *              (0 outside k = 1..MMRAG_MAX_K_DEEP; grows with n: it holds one query x n candidates) */
#define MMRAG_MAX_K_DEEP 4096
size_t mmrag_cosine_topk_deep_workspace_bytes(int B, int64_t n, int k);
int mmrag_cosine_topk_deep(const void *q, const void *corpus, int B, int64_t n, int d, int64_t ld,
                           int dtype, int k, int64_t row_offset, const uint32_t *alive_bits,
                           float *out_scores, int64_t *out_rows, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Exact re-scoring of candidate lists (FP8 collections: the scan plane over-fetches, the full-precision plane ranks).
 * For each of B queries and its C candidate rows (cand_rows dev [B, C] int64, rows below 2^31; a negative row ends
 * that query's list) the float32 dot product of q[b] with plane[row] over the first d columns, in mmrag_rows_dot's
 * summation order (bit-identical to it), then the best k ordered by (score desc, row asc), (-inf, -1) padded.
 *   q, plane   dev [B, ld] / [n, ld], dtype MMRAG_F32 / F16 / BF16 (MMRAG_F8E4M3 is rejected)
 *   1 <= k <= C <= MMRAG_MAX_RESCORE_CANDIDATES
 * One launch, one workgroup per query, no host synchronisation, no float atomics: the result depends neither on B
 * nor on the order in which the candidates are listed. */
#define MMRAG_MAX_RESCORE_CANDIDATES 4096
int mmrag_rescore_topk(const void *q, const void *plane, int64_t ld, int dtype, int d, const int64_t *cand_rows,
                       int B, int C, int k, float *out_scores, int64_t *out_rows, void *stream);

/* Merge G shards' local top-k (layout [G, B, k_in], as produced by an all-gather of
 * mmrag_cosine_topk outputs) into the global top-k [B, k].  Device version (one tiny
 * kernel) and host version (north star: "final host merge"); identical ordering rule.
 * Replaces nothing in the reference (it is single-process); it is the exchange step of the
 * row-sharded index. */
int mmrag_merge_topk(const float *scores, const int64_t *rows, int G, int B, int k_in, int k,
                     float *out_scores, int64_t *out_rows, void *stream);
int mmrag_merge_topk_host(const float *scores, const int64_t *rows, int G, int B, int k_in,
                          int k, float *out_scores, int64_t *out_rows);
/* Same merge over G rank blocks laid out [rows B*k_in i64 | scores B*k_in f32 | pad to 8 bytes]
 * each, i.e. the result of ONE all-gather of a packed per-rank buffer. */
int mmrag_merge_topk_host_packed(const void *blocks, int G, int B, int k_in, int k,
                                 float *out_scores, int64_t *out_rows);

/* ---------------------------------------------------------------------------------------
 * Store.  Replaces chromadb's  collection.add(embeddings=..., ...)  vector half
 * (app/utils/embedder.py:514-523): cast + copy `m` new float32 rows into the shard matrix
 * at row n_used (the id/metadata/document table stays on the host).
 *   corpus  dev [capacity, ld] dtype   new_rows dev [m, d] float32 (tightly packed)
 * The cast rounds to nearest even, pad columns [d, ld) of the written rows are set to zero and
 * nothing else is written.  m = 0 is a no-op with any pointers, null included (an empty device
 * tensor has none); every other bad argument returns MMRAG_EINVAL and launches nothing.
 * ------------------------------------------------------------------------------------- */
int mmrag_append_rows(void *corpus, int64_t capacity, int64_t ld, int dtype, int64_t n_used,
                      const float *new_rows, int64_t m, int d, void *stream);

/* Stable compaction after deletes (collection.delete, embedder.py:639-642):
 * dst[i, :] = src[keep_rows[i], :] for i < m.  dst and src must not overlap. */
int mmrag_gather_rows(void *dst, const void *src, int64_t ld, int dtype,
                      const int64_t *keep_rows, int64_t m, void *stream);

/* Fetch stored vectors as float32 (collection.get(ids, include=['embeddings']),
 * embedder.py:887-897): out[i, :d] = float(corpus[rows[i], :d]). */
int mmrag_fetch_rows_f32(const void *corpus, int64_t ld, int dtype, const int64_t *rows,
                         int64_t m, int d, float *out, void *stream);

/* Stream-ordered copy of a result block into (pinned) host memory: the last step of a query batch
 * (`results['ids'][0]` ... reach the host, embedder.py:604-609).  Thin wrapper so a serving loop can stay
 * on raw stream handles. */
int mmrag_copy_to_host_async(void *dst_host, const void *src_dev, size_t bytes, void *stream);


/* ---------------------------------------------------------------------------------------
 * Embed.  Replaces SentenceTransformer.encode(texts, batch_size=len(texts),
 * convert_to_numpy=True, normalize_embeddings=True)   app/utils/embedder.py:397-403
 * (tokenisation stays on the host; these entry points take token ids).
 * fp16 weights/activations, fp32 accumulate and fp32 LayerNorm / softmax / pooling statistics.
 * Sequences are PACKED: token t of sequence b is row cu_seqlens[b] + t; no padded tokens.
 * ------------------------------------------------------------------------------------- */
#define MMRAG_ACT_NONE 0
#define MMRAG_ACT_GELU 1       /* erf GELU (BERT) */
#define MMRAG_ACT_QUICK_GELU 2 /* x * sigmoid(1.702 x) (CLIP) */

#define MMRAG_ARCH_BERT 0  /* post-LN blocks, learned absolute positions, token-type 0 (pairs: per token), embedding LN */
#define MMRAG_ARCH_PRELN 1 /* pre-LN blocks (CLIP towers), final LN, bias-free projection */

#define MMRAG_POOL_MEAN 0  /* masked mean over the sequence's tokens (all-MiniLM-L6-v2) */
#define MMRAG_POOL_FIRST 1 /* first token: [CLS] (bge-base-en-v1.5, CLIP vision) */
#define MMRAG_POOL_SELECT 2 /* token sel[b] of each sequence (CLIP text: EOS position) */

typedef struct mmrag_encoder_desc {
    int32_t arch;
    int32_t n_layers, hidden, n_heads, intermediate, vocab, max_pos;
    int32_t pool, act, causal, normalize;
    int32_t out_dim; /* == hidden for BERT; projection width for MMRAG_ARCH_PRELN */
    float ln_eps;
    int32_t image, patch; /* vision tower only (mmrag_vit_forward): square image side, patch side */
} mmrag_encoder_desc;

/* Weight table `w` (device pointers; matrices fp16 stored [out_features][in_features], i.e.
 * the transpose of a torch Linear's .weight.T -- exactly nn.Linear.weight; biases and LayerNorm
 * parameters fp32):
 *   w[0] tok_emb [vocab,H]  w[1] pos_emb [max_pos,H]  w[2] type_emb row 0 [H] (NULL if none)
 *   w[3], w[4] embedding LayerNorm gamma, beta (both NULL for MMRAG_ARCH_PRELN text)
 *   then per layer l, at w[5 + 12 l ...]:
 *     wqkv [3H,H], bqkv [3H], wo [H,H], bo [H], ln1_g, ln1_b, w1 [I,H], b1 [I], w2 [H,I], b2 [H],
 *     ln2_g, ln2_b           (ln1 = attention LN, ln2 = MLP LN; pre- or post- per arch)
 *   MMRAG_ARCH_PRELN tail at w[5 + 12 L ...]: final_ln_g, final_ln_b, proj [out_dim, H]
 *
 *   ids, pos_ids  dev [T] int32 packed token ids / position ids
 *   cu_seqlens    dev [B+1] int32 row offsets, cu_seqlens[B] == T
 *   sel           dev [B] int32 (MMRAG_POOL_SELECT only)
 *   out           dev [B, out_dim] float32, L2-normalised when desc.normalize != 0 */
size_t mmrag_encoder_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_encoder_forward(const mmrag_encoder_desc *desc, const void *const *w, const int32_t *ids,
                          const int32_t *pos_ids, const int32_t *cu_seqlens, const int32_t *sel,
                          int64_t T, int B, int max_len, float *out, void *workspace,
                          size_t workspace_bytes, void *stream);

/* The encoder at the reference's own precision (opt-in; MMRAG_ENCODER_PRECISION=fp32).  SentenceTransformer.encode runs
 * in float32 (app/utils/embedder.py:397-403, device pick :204-210, no autocast anywhere); this entry point computes as
 * it does: float32 weights and activations, every contraction on the exact float32 matrix instruction
 * (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), LayerNorm / softmax / erf-GELU / pooling in float32.  BERT family
 * only.  Same arguments as mmrag_encoder_forward; the weight table has the same order with EVERY entry float32
 * (matrices [out_features][in_features]).  Throughput is bound by the float32 matrix rate (1/16 of fp16).
 *   mmrag_linear_f32   the GEMM of that mode on its own (parity tests): out = act(x . wt^T + bias) (+ resid) */
size_t mmrag_encoder_f32_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_encoder_forward_f32(const mmrag_encoder_desc *desc, const void *const *w, const int32_t *ids,
                              const int32_t *pos_ids, const int32_t *cu_seqlens, const int32_t *sel, int64_t T, int B,
                              int max_len, float *out, void *workspace, size_t workspace_bytes, void *stream);
int mmrag_linear_f32(const float *x, int64_t M, int K, const float *wt, int N, const float *bias, int act,
                     const float *resid, float *out, void *stream);

/* Cross-encoder re-ranking.  Fills in the reference's placeholder EmbeddingManager.rerank_results
 * (app/utils/embedder.py:834-859: "Re-ranking not implemented yet", truncation to top_k), whose docstring names a
 * cross-encoder: each (query, passage) pair is ONE packed sequence [CLS] a [SEP] b [SEP] scored by a
 * BertForSequenceClassification (e.g. cross-encoder/ms-marco-MiniLM-L-6-v2).
 * Embedding with segment ids -> the same encoder blocks as mmrag_encoder_forward / _f32 -> the [CLS] row ->
 * pooler tanh(W_p h + b_p) -> classifier W_c pooled + b_c, in float32 (one launch).
 *   desc        arch must be MMRAG_ARCH_BERT; desc.pool and desc.normalize are IGNORED (the head reads [CLS], raw)
 *   w           the weight table of mmrag_encoder_forward (fp16 mode) / mmrag_encoder_forward_f32 (fp32 mode), except
 *               w[2] = the whole token-type table [type_vocab >= 2, H] (rows 0 and 1 are read; type ids are clamped
 *               to 0..1, as ids are clamped to the vocabulary), and after the layers, at w[5 + 12 L ...]:
 *               pooler_w [H, H], pooler_b [H], cls_w [n_labels, H], cls_b [n_labels], all float32 in both modes
 *   n_labels    1..16
 *   ids, type_ids, pos_ids   dev [T] int32, packed as for the encoder (segment id 0 up to and including the first
 *               [SEP], 1 after it)
 *   out_logits  dev [B, n_labels] float32 (no sigmoid / softmax)
 *   workspace   >= mmrag_cross_encoder_workspace_bytes(desc, T, B) (fp32: the _f32 query), 16-byte aligned
 * Bad arguments return MMRAG_EINVAL, a short workspace MMRAG_EWORKSPACE.  Logits of a sequence do not depend on the
 * other sequences of the batch beyond the encoder's own GEMM tiling; identical calls give identical bits. */
size_t mmrag_cross_encoder_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_cross_encoder_forward(const mmrag_encoder_desc *desc, const void *const *w, int n_labels, const int32_t *ids,
                                const int32_t *type_ids, const int32_t *pos_ids, const int32_t *cu_seqlens, int64_t T,
                                int B, int max_len, float *out_logits, void *workspace, size_t workspace_bytes,
                                void *stream);
size_t mmrag_cross_encoder_f32_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_cross_encoder_forward_f32(const mmrag_encoder_desc *desc, const void *const *w, int n_labels,
                                    const int32_t *ids, const int32_t *type_ids, const int32_t *pos_ids,
                                    const int32_t *cu_seqlens, int64_t T, int B, int max_len, float *out_logits,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* Extractive reader (not in the reference): answer spans from a BertForQuestionAnswering head.  Each (question,
 * passage) pair is ONE packed sequence [CLS] question [SEP] passage [SEP] of at most MMRAG_MAX_READER_TOKENS tokens.
 *
 * mmrag_span_select (csrc/span_head.hip): ONE launch, one workgroup per sequence, over caller-supplied final hidden
 * states.  Start / end logits ls[t] = <hidden[t], qa_w[0]> + qa_b[0], le[t] = <hidden[t], qa_w[1]> + qa_b[1] (float32
 * accumulation, kept on chip), then per sequence b:
 *   out_lse[b][0], [1]  log-sum-exp of the start / of the end logits over position 0 ([CLS]) and the passage tokens
 *   out_null[b]         ls[0] + le[0], the score of "no answer in this passage"
 *   out_span[b][r], out_score[b][r], r < n_best: the candidates are all (i, j) with ctx_start <= i <= j <
 *       ctx_start + ctx_len and j - i < max_answer_tokens, scored ls[i] + le[j] (a float32 sum; a candidate must score
 *       above -inf).  Round r takes the best candidate that shares no token with a span of an earlier round: higher
 *       score first, then lower i, then lower j.  Spans are inclusive token offsets from the sequence's first token.
 *       A round without an eligible candidate gives (-1, -1) and -inf.
 *   hidden      dev [T, ld] fp16, 16-byte aligned; ld a multiple of 8, >= hidden_dim; hidden_dim a multiple of 64,
 *               at most 1024
 *   qa_w, qa_b  dev [2, hidden_dim], [2] float32 (qa_outputs.weight / .bias: row 0 start, row 1 end)
 *   cu_seqlens  dev [B + 1] int32; ctx_start, ctx_len dev [B] int32: the passage's tokens inside sequence b, counted
 *               from its first token ([CLS], the question and both [SEP]s excluded: ctx_start >= 1)
 *   max_answer_tokens  1..MMRAG_MAX_ANSWER_TOKENS;  n_best  1..MMRAG_MAX_READER_SPANS
 *   out_span    dev [B, n_best, 2] int32;  out_score dev [B, n_best];  out_null dev [B];  out_lse dev [B, 2] float32
 *   out_logits  dev [T, 2] float32 (start, end) or NULL: the logits are then never written to memory
 * Bad arguments return MMRAG_EINVAL before anything is launched; the device tables are not read by the host.  A sequence
 * that is empty, longer than MMRAG_MAX_READER_TOKENS or outside [0, T], or whose ctx_start / ctx_len fall outside it,
 * reads nothing and gets out_null = out_lse = NaN, spans (-1, -1) and scores -inf.  No atomics and no workspace: the
 * launch can be captured into a graph, identical calls give identical bits, and a sequence gives the same bits alone
 * or inside any batch.
 *
 * mmrag_reader_forward (csrc/encoder.hip): embedding with segment ids -> the encoder blocks of mmrag_encoder_forward
 * -> the span launch on the final hidden rows.  fp16 mode, MMRAG_ARCH_BERT only; desc.pool / normalize are IGNORED.
 *   w           the weight table of mmrag_cross_encoder_forward (w[2] = the two-row token-type table); after the
 *               layers, at w[5 + 12 L ...]: qa_w [2, H], qa_b [2], float32
 *   ids, type_ids, pos_ids   dev [T] int32, as for mmrag_cross_encoder_forward
 *   workspace   >= mmrag_reader_workspace_bytes(desc, T, B)
 * Bad arguments return MMRAG_EINVAL, a short workspace MMRAG_EWORKSPACE. */
#define MMRAG_MAX_READER_TOKENS 512
#define MMRAG_MAX_ANSWER_TOKENS 64
#define MMRAG_MAX_READER_SPANS 8
int mmrag_span_select(const void *hidden, int ld, int hidden_dim, const float *qa_w, const float *qa_b,
                      const int32_t *cu_seqlens, const int32_t *ctx_start, const int32_t *ctx_len, int64_t T, int B,
                      int max_answer_tokens, int n_best, int32_t *out_span, float *out_score, float *out_null,
                      float *out_lse, float *out_logits, void *stream);
size_t mmrag_reader_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_reader_forward(const mmrag_encoder_desc *desc, const void *const *w, const int32_t *ids,
                         const int32_t *type_ids, const int32_t *pos_ids, const int32_t *cu_seqlens,
                         const int32_t *ctx_start, const int32_t *ctx_len, int64_t T, int B, int max_len,
                         int max_answer_tokens, int n_best, int32_t *out_span, float *out_score, float *out_null,
                         float *out_lse, float *out_logits, void *workspace, size_t workspace_bytes, void *stream);

/* Vision tower (CLIP ViT-B/32 shape; BASELINE config 4 -- no reference behaviour):
 * patchify (+ fused uint8 -> normalised fp16 preprocessing) -> patch-embedding GEMM -> class token +
 * positions -> pre-LN -> the same pre-LN blocks / final LN / projection / L2 normalise as the text tower.
 * Weight table: w[0] patch kernel [H, 3*P*P] (conv weight flattened), w[1] pos_emb [NP+1, H],
 * w[2] class_embedding [H], w[3], w[4] pre-LN gamma/beta, layers and tail as for MMRAG_ARCH_PRELN.
 *   pixels       dev: fp16 [B,3,image,image] already normalised (MMRAG_PIXELS_F16_CHW) or uint8
 *                [B,image,image,3] raw crops (MMRAG_PIXELS_U8_HWC; CLIP mean/std applied on the GPU)
 *   cu_seqlens   dev [B+1] int32 = b * (NP+1)
 *   workspace    >= mmrag_encoder_workspace_bytes(desc, B*(NP+1), B) */
#define MMRAG_PIXELS_F16_CHW 0
#define MMRAG_PIXELS_U8_HWC 1
int mmrag_vit_forward(const mmrag_encoder_desc *desc, const void *const *w, const void *pixels, int pixel_kind,
                      const int32_t *cu_seqlens, int B, float *out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* Host-side WordPiece tokenizer (multi-threaded).  Replaces the tokenisation SentenceTransformer.encode performs
 * in native code (Hugging Face `tokenizers`) before the model runs -- app/utils/embedder.py:397-403.  BERT uncased
 * BasicTokenizer + greedy longest-match WordPiece over a caller-supplied vocabulary; strings travel as UTF-32.
 *   create   vocab token i = cps[offsets[i] .. offsets[i+1]), id = i; [CLS]/[SEP]/[UNK] looked up by name
 *            (defaults 101/102/100).  Returns NULL on error.
 *   encode   text i = cps[offsets[i] .. offsets[i+1]); ids [n, max_length] int32: row i holds
 *            [CLS] pieces... [SEP] truncated to max_length, lens[i] its length; n_threads host threads. */
void *mmrag_wordpiece_create(const uint32_t *cps, const int64_t *offsets, int n_tokens, int lower);
void mmrag_wordpiece_destroy(void *tokenizer);
int mmrag_wordpiece_encode_batch(const void *tokenizer, const uint32_t *cps, const int64_t *offsets, int n,
                                 int max_length, int32_t *ids, int32_t *lens, int n_threads);

/* Pair encoding for the cross-encoder (what CrossEncoder.predict's fast tokenizer does with (query, passage) pairs):
 * row i = [CLS] a_i [SEP] b_i [SEP] with type_ids 0 through the first [SEP] and 1 after it.  Over budget
 * max_length - 3 the pieces are cut by the fast tokenizer's LongestFirst rule: when the shorter side fits in half the
 * budget the longer side gets the rest; otherwise each side gets budget / 2 and an odd token goes to the longer side
 * (to b on equal lengths).  A text equal to the previous pair's text (the query of a batch) is tokenised once.
 *   ids, type_ids [n, max_length] int32 (entries past lens[i] untouched), lens [n]; max_length >= 3 */
int mmrag_wordpiece_encode_pairs(const void *tokenizer, const uint32_t *cps_a, const int64_t *offsets_a,
                                 const uint32_t *cps_b, const int64_t *offsets_b, int n, int max_length, int32_t *ids,
                                 int32_t *type_ids, int32_t *lens, int n_threads);

/* ---------------------------------------------------------------------------------------
 * Lexical retrieval (BM25).  The full-text leg the reference's Chroma store keeps beside its vector index
 * (an FTS5 table over every document); fused with the dense leg by VectorIndex.hybrid_query.
 *
 * Analyzer + lexicon (HOST, multi-threaded): BERT's text cleaning, whitespace split and CJK spacing; each word
 * str.lower() then its canonical decomposition KEEPING the combining marks; split at punctuation, which is dropped.
 * No stemming, no stop words.  The lexicon maps term strings to int32 ids in first-seen order.
 *   analyze_batch  text i = cps[offsets[i] .. offsets[i+1]); out_offsets [n+1]; pairs of text i are
 *                  (term_ids, tfs)[out_offsets[i] .. out_offsets[i+1]); dl [n] = its token count (unknown terms
 *                  included).  MMRAG_LEX_DOCUMENTS adds unseen terms and sorts each text's pairs by term id;
 *                  MMRAG_LEX_QUERIES adds nothing, drops unknown terms and keeps the order of first occurrence.
 *                  More than `capacity` pairs: MMRAG_EWORKSPACE with out_offsets filled in (call again with
 *                  capacity >= out_offsets[n]; adding terms twice is harmless). */
#define MMRAG_LEX_DOCUMENTS 0
#define MMRAG_LEX_QUERIES 1
void *mmrag_lexicon_create(void);
void mmrag_lexicon_destroy(void *lexicon);
int64_t mmrag_lexicon_size(const void *lexicon);
int mmrag_lexicon_analyze_batch(void *lexicon, const uint32_t *cps, const int64_t *offsets, int n, int mode,
                                int64_t *out_offsets, int32_t *term_ids, int32_t *tfs, int32_t *dl, int64_t capacity,
                                int n_threads);
/*   export         the code points of terms first_id .. first_id + count (ids are first-seen order, and so is the
 *                  lexicon's pool): term first_id + i = cps[offsets[i] .. offsets[i+1]), offsets [count+1] from 0.
 *                  More than `capacity` code points: MMRAG_EWORKSPACE with offsets filled in (offsets[count] is the
 *                  capacity to call again with).
 *   analyze_terms  the query mode that drops nothing: every DISTINCT term of text i in order of first occurrence,
 *                  term_ids[out_offsets[i] .. out_offsets[i+1]) (-1: not in the lexicon); term j of the whole batch is
 *                  out_cps[cp_offsets[j] .. cp_offsets[j+1]).  needed[0] / needed[1] are always set to the number of
 *                  terms / code points; more than term_capacity / cp_capacity: MMRAG_EWORKSPACE with out_offsets
 *                  filled in.  Adds nothing to the lexicon. */
int mmrag_lexicon_export(const void *lexicon, int32_t first_id, int32_t count, int64_t *offsets, uint32_t *cps,
                         int64_t capacity);
int mmrag_lexicon_analyze_terms(const void *lexicon, const uint32_t *cps, const int64_t *offsets, int n,
                                int64_t *out_offsets, int32_t *term_ids, int64_t *cp_offsets, uint32_t *out_cps,
                                int64_t term_capacity, int64_t cp_capacity, int64_t *needed, int n_threads);

/* Typo-tolerant term matching (all pointers dev): for each of n_patterns query terms, the max_expansions best lexicon
 * terms within its edit budget.  Term t = term_cps[term_off[t] .. term_off[t+1]), pattern p likewise.
 *   distance    optimal string alignment over code points: insert, delete, substitute and the transposition of two
 *               adjacent code points cost 1, no substring edited twice (osa("ca", "abc") = 3)
 *   candidates  terms with df[t] >= 1 and 1..MMRAG_FUZZY_MAX_LEN code points, at distance <= pat_edits[p] (0..2);
 *               a pattern longer than MMRAG_FUZZY_MAX_LEN has none
 *   order       smaller distance, then larger df, then lower term id: the 64-bit key
 *               (2 - dist) << 62 | df << 31 | (2^31 - 1 - id), selected by integer maxima (order-independent)
 *   out_terms, out_edits  [n_patterns, max_expansions] int32, best first, -1 padded
 *   workspace   mmrag_fuzzy_terms_workspace_bytes(...) bytes, 16-byte aligned; short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer, n_terms or n_patterns negative, max_expansions outside
 * 1..MMRAG_FUZZY_MAX_EXPANSIONS.  The edit budgets are device data: one outside 0..2 gives its pattern no candidates.
 * No host synchronisation. */
#define MMRAG_FUZZY_MAX_LEN 64
#define MMRAG_FUZZY_MAX_EXPANSIONS 16
size_t mmrag_fuzzy_terms_workspace_bytes(int n_terms, int n_patterns, int max_expansions);
int mmrag_fuzzy_terms(const int32_t *term_off, const uint32_t *term_cps, const int32_t *df, int n_terms,
                      const int32_t *pat_off, const uint32_t *pat_cps, const int32_t *pat_edits, int n_patterns,
                      int max_expansions, int32_t *out_terms, int32_t *out_edits, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Device index (all pointers dev).  Forward log: row r's postings are (fwd_term, fwd_tf)[fwd_off[r] .. fwd_off[r+1]),
 * sorted by term id (as MMRAG_LEX_DOCUMENTS produces them).  df [n_terms] counts the LIVE rows holding each term.
 *   df_update   df[t] += sign for every posting of rows[0 .. n_rows) (rows NULL: rows row0 .. row0 + n_rows); sign +-1.
 *               Integer atomics: the result does not depend on their order.
 *   csr_build   the term-major inverted index of rows [0, n): post_row / post_tf [term_off[t] .. term_off[t+1]) hold
 *               term t's postings sorted by row (dead rows included: the alive bits filter them).  term_off [n_terms+1],
 *               post_* [fwd_off[n]].  Counting sort (histogram, scan, scatter) then a per-term sort by row.
 *   bm25_topk   for query b with terms q_terms[q_off[b] .. q_off[b+1]) (distinct, in order of first occurrence):
 *                 score(d) = sum_t idf_t * tf (k1 + 1) / (tf + k1 (1 - b + b dl_d / avgdl)),
 *                 idf_t = ln(1 + (N - df_t + 0.5) / (df_t + 0.5)),  N = n_live,  avgdl = sum_dl / N,
 *               float32, the terms added in query order.  Rows with a score > 0 (at least one query term), set in
 *               alive_bits (NULL = every row) compete; out [B, k] score desc, ties to the lower row, (-inf, -1) padded.
 *               k 1..MMRAG_MAX_K_DEEP.  Synchronises `stream` once to read the per-query match counts (a query
 *               whose matches overflow its candidate buffer is re-run alone into a buffer of n slots).
 *   rows_dot    out[i] = <q[qi[i]], corpus[rows[i]]> over the first d columns, float32 (the cosine of a row the dense
 *               leg did not return). */
int mmrag_lexical_df_update(const int64_t *fwd_off, const int32_t *fwd_term, const int64_t *rows, int64_t row0,
                            int64_t n_rows, int sign, int32_t *df, void *stream);
size_t mmrag_lexical_csr_build_workspace_bytes(int64_t n, int n_terms);
int mmrag_lexical_csr_build(const int64_t *fwd_off, const int32_t *fwd_term, const int32_t *fwd_tf, int64_t n,
                            int64_t n_postings, int n_terms, int64_t *term_off, int32_t *post_row, int32_t *post_tf,
                            void *workspace, size_t workspace_bytes, void *stream);
size_t mmrag_bm25_topk_workspace_bytes(int B, int64_t n, int k);
int mmrag_bm25_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_tf, const int32_t *dl,
                    const int32_t *df, int n_terms, int64_t n, const int32_t *q_off, const int32_t *q_terms, int B,
                    int64_t n_live, int64_t sum_dl, float k1, float b, int k, const uint32_t *alive_bits,
                    float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream);
int mmrag_rows_dot(const void *q, const void *corpus, int64_t ld, int dtype, int d, const int32_t *qi,
                   const int64_t *rows, int64_t m, float *out, void *stream);

/* Phrase queries: a positional index beside the forward log (csrc/phrase.hip; tests/phrase_ref.py restates it).
 *
 * analyze_positions (HOST)  mmrag_lexicon_analyze_batch in MMRAG_LEX_DOCUMENTS mode -- the same pairs, ids, dl and
 *               lexicon growth -- that also writes every pair's token positions (0-based token indices of the text),
 *               ascending, concatenated in pair order: sum(dl) ints for the batch.  *pos_needed is always set to that
 *               number.  More than `capacity` pairs or `pos_capacity` positions: MMRAG_EWORKSPACE with out_offsets, dl
 *               and *pos_needed filled in (call again with enough of both).
 *
 * Positions plane (dev): pos_off [P + 1] int64, the prefix sum of fwd_tf over the P forward postings; forward posting i
 * stands at the token positions pos[pos_off[i] .. pos_off[i+1]), ascending.
 *
 * Phrase tables (dev): phrase p has the terms ph_terms[ph_off[p] .. ph_off[p+1]) (1..MMRAG_MAX_PHRASE_TERMS, repeats
 * kept) and the DRIVER term ph_driver[p]: the one of its terms with the fewest postings (the caller chooses; any term
 * of the phrase gives the same result), or -1 for a phrase that occurs nowhere.  Query b holds the phrases
 * q_ph[q_ph_off[b] .. q_ph_off[b+1]) (distinct, at most MMRAG_MAX_QUERY_PHRASES).  ptf_off [n_phrases + 1] int64: the
 * prefix sum of the drivers' postings counts (0 for a driver of -1).  The tables are device data: the caller states the
 * longest phrase (max_terms) and the most phrases of one query (max_phrases), and the kernels read no more than those.
 *
 *   phrase_match  the phrase (t_0 .. t_m-1) occurs at start i of a row's token sequence T under `slop` s when
 *               T[i] = t_0 and positions i = p_0 < p_1 < .. < p_m-1 exist with T[p_j] = t_j and
 *               p_m-1 - p_0 - (m - 1) <= s; tf_p(row) counts such starts (overlaps count; s = 0 is the contiguous
 *               phrase).  For posting i of the driver's CSR list (row r = post_row[term_off[driver] + i]):
 *               ptf[ptf_off[p] + i] = tf_p(r), 0 for a row not set in alive_bits (NULL = every row).  ph_rows[p] = the
 *               number of rows with tf_p >= 1 (integer atomics: order-free).  With `bitmaps` ([B, mmrag_filter_words(n)]
 *               uint32, bit r & 31 of word r >> 5): query b's rows holding EVERY one of its phrases; a query without
 *               phrases gets every row below n.  max_driver_postings: the longest driver list (sizes the grid; postings
 *               beyond it are not visited).  No host synchronisation.
 *   bm25_phrase_topk  mmrag_bm25_topk with phrases as further clauses: after query b's loose terms, in q_ph order, each
 *               phrase adds idf_p * tf_p (k1 + 1) / (tf_p + k1 (1 - b + b dl / avgdl)), idf_p = the sum of its terms'
 *               idf in phrase order (a repeated term counts each time), tf_p from `ptf` as phrase_match wrote it.
 *               require != 0: a query that has phrases returns only rows with tf_p >= 1 for every one of them (its loose
 *               terms only add score); require == 0 and queries without phrases: rows with a score > 0.  Order, padding,
 *               k, alive_bits, the one synchronisation and the overflow re-run as mmrag_bm25_topk; a batch without
 *               phrases returns bit for bit what mmrag_bm25_topk returns.
 * MMRAG_EINVAL before anything is launched: a null pointer, negative counts, B < 1, k outside 1..MMRAG_MAX_K_DEEP, slop
 * outside 0..MMRAG_MAX_PHRASE_SLOP, max_terms above MMRAG_MAX_PHRASE_TERMS, max_phrases above MMRAG_MAX_QUERY_PHRASES. */
#define MMRAG_MAX_PHRASE_TERMS 8
#define MMRAG_MAX_QUERY_PHRASES 4
#define MMRAG_MAX_PHRASE_SLOP 16
int mmrag_lexicon_analyze_positions(void *lexicon, const uint32_t *cps, const int64_t *offsets, int n,
                                    int64_t *out_offsets, int32_t *term_ids, int32_t *tfs, int32_t *dl,
                                    int64_t capacity, int32_t *positions, int64_t pos_capacity, int64_t *pos_needed,
                                    int n_threads);
int mmrag_phrase_match(const int64_t *fwd_off, const int32_t *fwd_term, const int64_t *pos_off, const int32_t *pos,
                       int64_t n, const int64_t *term_off, const int32_t *post_row, const int32_t *ph_off,
                       const int32_t *ph_terms, const int32_t *ph_driver, const int64_t *ptf_off, int n_phrases,
                       int max_terms, int64_t max_driver_postings, int slop, const uint32_t *alive_bits, int32_t *ptf,
                       int32_t *ph_rows, const int32_t *q_ph_off, const int32_t *q_ph, int B, int max_phrases,
                       uint32_t *bitmaps, void *stream);
size_t mmrag_bm25_phrase_topk_workspace_bytes(int B, int64_t n, int k);
int mmrag_bm25_phrase_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_tf, const int32_t *dl,
                           const int32_t *df, int n_terms, int64_t n, const int32_t *q_off, const int32_t *q_terms,
                           int B, const int32_t *q_ph_off, const int32_t *q_ph, const int32_t *ph_off,
                           const int32_t *ph_terms, const int32_t *ph_driver, const int64_t *ptf_off,
                           const int32_t *ptf, int n_phrases, int max_terms, int max_phrases, int require,
                           int64_t n_live, int64_t sum_dl, float k1, float b, int k, const uint32_t *alive_bits,
                           float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream);

/* Significant terms: which terms set a group of rows apart from the collection (csrc/terms.hip; tests/terms_ref.py
 * restates it).  All pointers dev.  term_off / post_row / df are mmrag_lexical_csr_build's CSR of rows [0, n) and the
 * live df; group [n] labels every row with its group 0 .. n_groups-1 or -1 for none (dead rows must be -1; a label at
 * or above n_groups counts for nothing); group_size [n_groups] is the number of rows labelled g; term_bits (NULL: every
 * term) holds bit t & 31 of word t >> 5 for every term that may be returned.
 *   group_terms  for group g and term t, with fg = the rows of g holding t (a posting counts once, whatever its tf),
 *               fgp = (float)fg / (float)group_size[g] and bgp = (float)df[t] / (float)n_live, the pair qualifies when
 *               group_size[g] > 0, df[t] > 0, fg >= min_count, t is set in term_bits and fgp > bgp; its score is the
 *               JLH measure (fgp - bgp) * (fgp / bgp), float32, every operation rounded once.  out [n_groups, top]:
 *               each group's best qualifying terms, score desc, ties to the lower term id, (-inf, -1) padded;
 *               out_counts holds fg of every returned pair and 0 on padding.  Terms with df < min_count are dropped
 *               without a visit of their postings (df bounds every fg).  One launch counts MMRAG_TERM_GROUP_WINDOW
 *               consecutive groups in on-chip histograms; more groups take more launches over the same CSR, and the
 *               workspace is sized for one launch, not for n_groups.  Synchronises `stream` once per launch to read
 *               the per-group candidate counts (a group whose qualifying terms overflow its candidate buffer is
 *               counted again alone into a buffer of n_terms slots); not at all when n_terms fits the buffer.
 * MMRAG_EINVAL before anything is launched: a null pointer, n_groups outside 1..MMRAG_MAX_TERM_GROUPS, top outside
 * 1..MMRAG_MAX_K_DEEP, min_count < 1, a negative n, n_terms or n_live, n_live > n.  MMRAG_EWORKSPACE: a workspace below
 * mmrag_group_terms_workspace_bytes (0 for arguments the call refuses).  n, n_live or n_terms of 0: empty outputs. */
#define MMRAG_MAX_TERM_GROUPS 4096
#define MMRAG_TERM_GROUP_WINDOW 256
size_t mmrag_group_terms_workspace_bytes(int n_groups, int n_terms, int top);
int mmrag_group_terms(const int64_t *term_off, const int32_t *post_row, const int32_t *df, int n_terms, int64_t n,
                      const int32_t *group, const int32_t *group_size, int n_groups, int64_t n_live,
                      const uint32_t *term_bits /* NULL: every term */, int min_count, int top,
                      float *out_scores, int64_t *out_terms, int32_t *out_counts,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Diversified retrieval: maximal-marginal-relevance (MMR) selection of k of a query's C dense hits (what LangChain's
 * max_marginal_relevance_search(k, fetch_k, lambda_mult) does over a Chroma collection).  The reference has no
 * counterpart: app/utils/embedder.py hands the first top_k hits of collection.query to the generator as they come.
 * One launch, one workgroup per query, everything in LDS; no atomics on global memory, no host synchronisation (the
 * call can be captured into a graph).
 *
 * Definition, for one query:
 *   - the candidates c_0 .. c_{C-1} are cand_rows[b, :] in the search's own order (score descending, ties to the lower
 *     row); rel_i = cand_scores[b, i] exactly as given; a (-inf, -1) padded tail is allowed: the list ends at its first
 *     row < 0 and the query selects from what it has;
 *   - sim(i, j) = float32 dot product of the stored rows of c_i and c_j over the first d columns, elements widened to
 *     float32, summed in one fixed order that does not depend on B, C, k or the grid (the row is cut into 16-byte
 *     chunks; lane l of a 64-lane wave adds the elements of chunks l, l + 64, ... in ascending order into one
 *     accumulator with fmaf; the 64 accumulators are added by the xor butterfly 32, 16, 8, 4, 2, 1);
 *   - step 0 picks c_0; step t >= 1 picks the not yet picked i that maximises
 *         v_i = fl(fl(lambda * rel_i) - fl(fl(1 - lambda) * max_{j in S} sim(i, j)))     (float32, S = the picks so far)
 *     ties to the lower i (the better dense rank); selection stops after k picks or when the candidates run out;
 *   - output in pick order: out_scores = rel, out_rows = the row, out_pos = i, out_mmr = v at the time of the pick
 *     (rel_0 for step 0); unused slots are (-inf, -1, -1, -inf).
 * lambda = 1 reproduces the first k candidates; lambda = 0 is pure diversity after the first pick.
 *
 *   corpus       dev [*, ld] rows of `dtype`, 16-byte aligned, ld * element size a multiple of 16 (any ld the index
 *                uses); every cand_rows entry >= 0 must be a row of it (rows are not checked against a count)
 *   cand_scores  dev [B, C] float32      cand_rows  dev [B, C] int64
 *   out_*        dev [B, k]: float32, int64, int32, float32
 *   workspace    >= mmrag_mmr_select_workspace_bytes(B, C, d, dtype) bytes, which is 0 today (NULL is accepted)
 * MMRAG_EINVAL unless 1 <= k <= C <= MMRAG_MAX_MMR_CANDIDATES, 0 <= lambda <= 1 (NaN is rejected) and dtype is known;
 * arguments are checked before any HIP call. */
#define MMRAG_MAX_MMR_CANDIDATES 1024
size_t mmrag_mmr_select_workspace_bytes(int B, int C, int d, int dtype);
int mmrag_mmr_select(const void *corpus, int64_t ld, int dtype, int d, const float *cand_scores,
                     const int64_t *cand_rows, int B, int C, int k, float lambda, float *out_scores, int64_t *out_rows,
                     int32_t *out_pos, float *out_mmr, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Grouping of search hits by a per-row key ("group by" / "collapse" of comparable vector stores): the first n_groups
 * groups of a query's candidate list with up to group_size members each -- the top documents and the best passages of
 * each, where the rows are chunks and the key is their document.  The reference has no counterpart: it ranks chunks.
 * One launch, one workgroup per query, no workspace, no host synchronisation (the call can be captured into a graph),
 * no float atomics; identical bits run to run, and the same result whatever else is in the batch.
 *
 * Definition.  For one query, take its candidate list c_0 .. c_{C-1} exactly as search() returns it: score descending,
 * ties to the lower row.  The list ends at the first row < 0.
 *   Group key
 *   - Each candidate row has a group ordinal g = group_of_row[row], an int32.
 *   - g < 0, or a row >= n_rows, means the row has no key.  Such a row is a group of its own, reported as ordinal -1.
 *     It never merges with another row, and nothing read is out of bounds.
 *   Group order
 *   - Groups are ranked by first appearance in the list.
 *   - A group is therefore ranked by its best member's score, with ties to the lower row.
 *   Members
 *   - A group's members are its candidates in list order.
 *   - Only the first group_size (S) are kept.
 *   Output
 *   - The output is the first n_groups (G) groups.
 *   - Per query it holds:
 *       out_scores [G,S] float32, the input scores copied bit for bit
 *       out_rows   [G,S] int64
 *       out_pos    [G,S] int32, the position in the candidate list
 *       out_group  [G]   int32
 *       out_info   [2]   int32 = (groups found, capped at G; valid candidates)
 *   - Unused slots hold (-inf, -1, -1), and -2 in out_group.
 * Nothing here is floating-point arithmetic: the result is exact.
 *
 *   scores  dev [B, C] float32      rows  dev [B, C] int64      group_of_row  dev [n_rows] int32 (NULL only with n_rows 0)
 *   out_scores, out_rows, out_pos  dev [B, G, S]      out_group  dev [B, G]      out_info  dev [B, 2]
 * MMRAG_EINVAL unless B >= 1, 1 <= C <= MMRAG_MAX_GROUP_CANDIDATES, 1 <= n_groups <= MMRAG_MAX_GROUPS,
 * 1 <= group_size <= MMRAG_MAX_GROUP_SIZE and n_rows >= 0; arguments are checked before any HIP call. */
#define MMRAG_MAX_GROUP_CANDIDATES 4096
#define MMRAG_MAX_GROUPS 256
#define MMRAG_MAX_GROUP_SIZE 16
int mmrag_group_select(const float *scores, const int64_t *rows, int B, int C, const int32_t *group_of_row,
                       int64_t n_rows, int n_groups, int group_size, float *out_scores, int64_t *out_rows,
                       int32_t *out_pos, int32_t *out_group, int32_t *out_info, void *stream);

/* ---------------------------------------------------------------------------------------
 * Multi-query retrieval ("query expansion", "RAG-fusion"): the ranked lists that several phrasings of one question got
 * from the search, fused into one ranking, so that a row several phrasings agree on outranks a row only one of them
 * likes.  The reference has no counterpart: it searches one phrasing.
 * One launch, one workgroup per group (one question), everything in LDS; no workspace, no atomics on global memory, no
 * host synchronisation (the call can be captured into a graph); identical bits run to run, and a group's result does
 * not depend on G, on the grid, or on what else is in the call.
 *
 * Definition.  Group g owns the lists list_off[g] .. list_off[g + 1] - 1 (none is allowed); list l of the group is its
 * l-th, a group-local index.  For one group:
 *   List length and duplicates
 *   - List l ends at its first row < 0; what follows in the list is not read as entries.
 *   - Entry (l, p) at 0-based position p has rank p + 1.
 *   - If a row occurs more than once in one list, only its first occurrence counts.
 *   Contribution of entry (l, p), w_l the list's weight (1.0 when weights is NULL)
 *   - MMRAG_FUSE_RRF: c(l, p) = w_l / (float)(rrf_k + p + 1), ONE correctly rounded float32 division.
 *   - MMRAG_FUSE_MAX: c(l, p) = fl(w_l * score(l, p)), one float32 multiplication.
 *   Fused score of a row, over the lists that returned it in ascending l
 *   - RRF: the first contribution, then each further one added to it in float32, one list after the other.
 *   - MAX: the largest contribution (a later one replaces the value only where it compares greater).
 *   Per row
 *   - best: the largest input score of the row over its lists, copied bit for bit (a later list replaces it only
 *     where its score compares greater); best_list: the list that gave it, so ties go to the lower list.
 *   - count: the number of lists that returned the row.
 *   Order
 *   - fused descending, then best descending, then row ascending.
 *   - Floats compare as floats: -0.0 equals 0.0, and such a pair falls through to the next key.
 *   Output, per group
 *   - out_fused [n] float32, out_rows [n] int64, out_best [n] float32, out_best_list [n] int32, out_count [n] int32:
 *     the first n rows of that order;
 *     out_info [2] int32 = (distinct rows found, valid entries read = the sum of the list lengths).
 *   - Unused slots hold (-inf, -1, -inf, -1, 0).
 * Scores of valid entries and the weights must be finite (a NaN has no place in the order); weights may be zero or
 * negative.  Rows are full int64 in [0, 2^63 - 1).
 *
 *   scores  dev [L, C] float32     rows  dev [L, C] int64: the lists as mmrag_cosine_topk / _deep wrote them (score
 *           descending, (-inf, -1) padded tail allowed; the order is not checked and nothing depends on it)
 *   list_off  dev [G + 1] int32, ascending, list_off[0] = 0, list_off[G] = L.  A group must own at most
 *           MMRAG_MAX_FUSE_LISTS lists; the offsets are on the device, so the CALLER checks that.  Nothing is read out
 *           of bounds whatever they hold: offsets outside [0, L] or descending make the group empty, and of a group
 *           with more lists only the first MMRAG_MAX_FUSE_LISTS are read.
 *   weights   dev [L] float32 or NULL
 *   out_*     dev [G, n]      out_info  dev [G, 2]
 * MMRAG_EINVAL unless G >= 1, L >= 0, 1 <= C <= MMRAG_MAX_FUSE_CANDIDATES, 1 <= n <= MMRAG_MAX_FUSE_RESULTS,
 * rrf_k >= 0 and method is MMRAG_FUSE_RRF or MMRAG_FUSE_MAX; arguments are checked before any HIP call. */
#define MMRAG_MAX_FUSE_LISTS 16
#define MMRAG_MAX_FUSE_CANDIDATES 256
#define MMRAG_MAX_FUSE_RESULTS 4096
#define MMRAG_FUSE_RRF 0
#define MMRAG_FUSE_MAX 1
int mmrag_fuse_select(const float *scores, const int64_t *rows, int L, int C, const int32_t *list_off, int G,
                      const float *weights, int method, int rrf_k, int n, float *out_fused, int64_t *out_rows,
                      float *out_best, int32_t *out_best_list, int32_t *out_count, int32_t *out_info, void *stream);

/* ---------------------------------------------------------------------------------------
 * Near-duplicate detection: the exact all-pairs threshold self-join of a row matrix.  The reference has no counterpart:
 * app/utils/embedder.py stores every chunk of every upload again (ids are f"{doc_id}_{item id}", :514-523).
 * X . X^T over the upper triangle in 128 x 128 tiles; the N x N matrix is never written.
 *
 * Contract
 *   - emits every pair (i, j) with 0 <= i < j < n, both rows alive and dot(row_i, row_j) >= threshold, each once, in no
 *     defined order: out_pairs[s] = (i, j), out_scores[s] = the dot;
 *   - the dot is over the stored rows (unit rows => cosine), float32 accumulation in one fixed order: a pair's score
 *     bits depend on its two rows and d only, not on n, the bitmap, the capacity or the grid;
 *   - *count receives the TOTAL number of qualifying pairs, exact also above `capacity`; then exactly `capacity`
 *     distinct qualifying pairs are stored and nothing is written past them;
 *   - one launch after a memset of *count, no host synchronisation, no workspace; the only global atomics are integer
 *     adds on *count (the call can be captured into a graph).
 *
 *   rows        dev [n, ld] of `dtype` MMRAG_F32 / F16 / BF16, pad columns zero; MMRAG_F8E4M3 returns
 *               MMRAG_EUNSUPPORTED (an FP8 collection is joined on its re-scoring plane)
 *   ld          mmrag_padded_dim(d, dtype) or a larger width of whole 128-byte slabs
 *   alive       dev, optional (NULL = every row): bit r & 31 of word r >> 5, at least (n + 31) / 32 words
 *   out_pairs   dev [capacity, 2] int64, 16-byte aligned      out_scores  dev [capacity] float32
 *   count       dev, one unsigned 64-bit integer; zeroed by the call
 * MMRAG_EINVAL before anything is launched: a null pointer, n < 0 or above 2^23, d <= 0, ld < d, capacity < 0 or above
 * MMRAG_MAX_JOIN_PAIRS, a threshold that is NaN or <= 0.  n < 2 succeeds with count 0. */
#define MMRAG_MAX_JOIN_PAIRS (1 << 26)
int mmrag_sim_join(const void *rows, int64_t n, int64_t ld, int dtype, int d, const uint32_t *alive, float threshold,
                   int64_t *out_pairs, float *out_scores, int64_t capacity, unsigned long long *count, void *stream);

/* ---------------------------------------------------------------------------------------
 * Topic clustering: the two device steps of a spherical k-means (Lloyd) iteration over the stored unit rows.  The
 * reference has no counterpart: nothing in it describes what a collection holds.  The host loop (rounding the master
 * centroids, the sort by cluster, the re-normalisation, the stop rule) is multimodal_rag_amd/index.py
 * VectorIndex.cluster.
 *
 * mmrag_kmeans_assign: the nearest centroid of every row, X . C^T in 128 x 128 tiles with an arg-max epilogue; the
 * [n, k] scores are never written.
 * Contract
 *   - for an alive row r: out_score[r] = max over c of dot(rows[r], centroids[c]) (float32 accumulation in one fixed
 *     K order), out_assign[r] = the LOWEST c that attains it; a row whose alive bit is clear gets (-1, -inf);
 *   - a row's two outputs depend on that row, the centroid matrix and d only: not on n, the bitmap, the grid or the
 *     workgroup that ran it;
 *   - one launch, no workspace, no host synchronisation, no atomics (the call can be captured into a graph).
 *
 *   rows        dev [n, ld] of `dtype` MMRAG_F32 / F16 / BF16, pad columns zero; MMRAG_F8E4M3 returns
 *               MMRAG_EUNSUPPORTED (an FP8 collection is clustered on its re-scoring plane)
 *   centroids   dev [k, ld], same dtype and ld, pad columns zero (the caller rounds its float32 master centroids)
 *   ld          mmrag_padded_dim(d, dtype) or a larger width of whole 128-byte slabs
 *   alive       dev, optional (NULL = every row): bit r & 31 of word r >> 5, at least (n + 31) / 32 words
 *   out_assign  dev [n] int32      out_score  dev [n] float32
 * MMRAG_EINVAL before anything is launched: a null pointer, n < 0 or >= 2^31, k < 1 or above MMRAG_MAX_CLUSTERS,
 * d <= 0, ld < d.  n == 0 succeeds.
 *
 * mmrag_cluster_sums: out_sums[c, :] = the float32 sum of the rows order[seg_off[c] .. seg_off[c + 1]), c < k.
 *   - every element of out_sums is written; an empty segment gives zeros;
 *   - deterministic: member i of a segment goes to partial sum i % 32, each partial adds its members in segment order,
 *     and the 32 partials are added by the fixed tree of strides 16, 8, 4, 2, 1.  A cluster's bits depend on its own
 *     member rows in that order only: not on the other clusters, n or the grid.  No atomics, no workspace;
 *   - one launch, no host synchronisation.
 *
 *   rows, ld, dtype, d   as above
 *   order       dev [seg_off[k]] int32 row numbers, every one a row of `rows` (not checked against a count)
 *   seg_off     dev [k + 1] int64, non-decreasing offsets into `order`
 *   out_sums    dev [k, d] float32
 * MMRAG_EINVAL / MMRAG_EUNSUPPORTED as for mmrag_kmeans_assign. */
#define MMRAG_MAX_CLUSTERS 4096
int mmrag_kmeans_assign(const void *rows, int64_t n, int64_t ld, int dtype, int d, const void *centroids, int k,
                        const uint32_t *alive, int32_t *out_assign, float *out_score, void *stream);
int mmrag_cluster_sums(const void *rows, int64_t ld, int dtype, int d, const int32_t *order, const int64_t *seg_off,
                       int k, float *out_sums, void *stream);

/* Document-scoped top-k (csrc/scoped.hip): a batch of queries in ONE masked scan, each query seeing only the rows whose
 * group ordinal (e.g. document) is in its own scope.  VectorIndex.scoped_search.
 *
 * A scope is a set of group ordinals.  Query b sees row r iff r < n, r's alive bit is set (when alive_bits is given)
 * and group_of_row[r] is in scope scope_of_query[b]; a row with ordinal -1 is in no scope.
 * Contract
 *   - out_scores / out_rows [B, k] as mmrag_cosine_topk_deep's: score descending, ties to the lower row,
 *     row + row_offset, (-inf, -1) padded; an empty scope, or one whose rows are all dead, gives padding only;
 *   - a score's bits depend on the query row, the stored row and d alone (one fixed K order): not on the batch, the
 *     scopes or the grid;
 *   - a 128-row tile of stored rows whose ordinals no query of a 128-query tile can see is not fetched for that tile;
 *   - every visible row is a candidate: a query has candidate slots for 32 k rows, at least 16384.  With
 *     max_candidates at or below that nothing can overflow and the call does not synchronise; otherwise `stream` is
 *     synchronised once to read the counts and a query with more visible rows is produced again alone.
 *
 *   q, rows         dev [B, ld] and [n, ld] of one `dtype` MMRAG_F32 / F16 / BF16 and one ld (mmrag_padded_dim or a
 *                   larger width of whole 128-byte slabs), pad columns zero; MMRAG_F8E4M3 returns MMRAG_EUNSUPPORTED (an FP8
 *                   collection is searched by scope on its re-scoring plane)
 *   k               1..MMRAG_MAX_K_DEEP
 *   alive_bits      dev, optional (NULL = every row): bit r & 31 of word r >> 5
 *   group_of_row    dev [n] int32 ordinals in -1..n_groups-1
 *   scope_of_query  dev [B] int32 in 0..S-1
 *   scope_off       dev [S + 1] int32 ascending offsets into scope_groups; scope s = scope_groups[scope_off[s] ..
 *                   scope_off[s + 1]), at most MMRAG_MAX_SCOPE_GROUPS ordinals, ascending
 *   max_candidates  the caller's upper bound on the rows any ONE scope holds (n if unknown); a scope that holds more
 *                   loses candidates
 *   workspace       dev, >= mmrag_scoped_topk_workspace_bytes(B, n, k, n_groups) bytes (0 for arguments out of range),
 *                   16-byte aligned
 * MMRAG_EINVAL before anything is launched: a null pointer, B < 1, S < 1, n < 0 or >= 2^31, k out of range, d <= 0,
 * ld < d, n_groups < 0, max_candidates < 0.  The scope tables live on the device and are not read by the host: a
 * scope_of_query outside 0..S-1, a scope longer than MMRAG_MAX_SCOPE_GROUPS and an ordinal outside 0..n_groups-1 match
 * nothing (the Python wrapper checks the host copies it is given). */
#define MMRAG_MAX_SCOPE_GROUPS 64
size_t mmrag_scoped_topk_workspace_bytes(int B, int64_t n, int k, int n_groups);
int mmrag_scoped_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                      int64_t row_offset, const uint32_t *alive_bits, const int32_t *group_of_row, int n_groups,
                      const int32_t *scope_of_query, int S, const int32_t *scope_off, const int32_t *scope_groups,
                      int64_t max_candidates, float *out_scores, int64_t *out_rows, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Boosted top-k (csrc/boosted.hip): a batch of queries ranked by cosine plus a per-row score prior, applied inside ONE
 * exact scan.  VectorIndex.boosted_search.
 *
 * final[b][r] = fmaf(weight[b], prior[r], dot[b][r]).  Row r is a candidate iff r < n and its alive bit is set (when
 * alive_bits is given).
 * Contract
 *   - one rounding: dot is the float32 accumulation of the pair-tile body's fixed K order, so a dot's bits depend on the
 *     query row, the stored row and d alone and equal mmrag_scoped_topk's for the same two rows; final's bits depend on
 *     those plus weight[b] and prior[r]: not on the batch, the grid, the threshold or whether bound passes ran;
 *   - out_scores / out_rows [B, k] as mmrag_cosine_topk_deep's: final descending, ties to the lower row,
 *     row + row_offset, (-inf, -1) padded;
 *   - out_boost [B, k], optional (NULL allowed): weight[b] * prior[row], the exact float32 product, 0.0 in padding;
 *   - with weight[b] == 0 a query's result is the plain exact top-k with this body's dot bits;
 *   - exact under ANY finite prior: when n exceeds the candidate slots of a query (32 k, at least 16384) a sampled
 *     lower bound on the k-th final is staged first (the k-th best of any subset of live rows is at most the true k-th),
 *     and only finals at or above it are kept;
 *   - at most one stream synchronisation per call, and only when n exceeds the candidate slots: the counts are read
 *     once and a query with more survivors than slots is produced again alone.
 *
 *   q, rows         as mmrag_scoped_topk's: dev [B, ld] and [n, ld] of one `dtype` MMRAG_F32 / F16 / BF16 and one ld of
 *                   whole 128-byte slabs, pad columns zero; MMRAG_F8E4M3 returns MMRAG_EUNSUPPORTED (an FP8 collection is
 *                   searched with a prior on its re-scoring plane)
 *   k               1..MMRAG_MAX_K_DEEP
 *   alive_bits      dev, optional (NULL = every row): bit r & 31 of word r >> 5
 *   prior           dev [n] float32, finite
 *   weight          dev [B] float32, finite
 *   workspace       dev, >= mmrag_boosted_topk_workspace_bytes(B, n, k) bytes (0 for arguments out of range), 16-byte
 *                   aligned; short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer (the optional ones aside), B < 1, n < 0 or >= 2^31, k out of
 * range, d <= 0, ld < d or not whole slabs.  prior and weight live on the device and are not read by the host (the
 * Python wrapper checks the host copies it uploads); a non-finite value gives an unspecified ranking. */
size_t mmrag_boosted_topk_workspace_bytes(int B, int64_t n, int k);
int mmrag_boosted_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                       int64_t row_offset, const uint32_t *alive_bits, const float *prior, const float *weight,
                       float *out_scores, int64_t *out_rows, float *out_boost, void *workspace, size_t workspace_bytes,
                       void *stream);

/* Recommend top-k (csrc/recommend.hip): "more like these, less like those" -- a batch of requests, each a group of
 * signed example vectors, ranked inside ONE exact scan.  VectorIndex.recommend_search.
 *
 * A request owns MMRAG_MAX_RECOMMEND_EXAMPLES slots.  Each holds a unit vector with a sign: +1 positive, -1 negative,
 * 0 unused.  For a live stored row x (r < n, alive bit set when alive_bits is given):
 *   pos   = max over the request's positive examples e of <e, x>
 *   neg   = max over its negative examples e of <e, x>          (no negatives: neg = 0)
 *   final = fmaf(-w, max(neg, 0), pos)                           one rounding, w >= 0 per request
 * max(neg, 0): a row is never rewarded for being unlike a negative.  With no negatives final = pos, "nearest to any of
 * these".  A request needs at least one positive; one without gets padding only.
 * Contract
 *   - a dot is the float32 accumulation of the pair-tile body's fixed K order: its bits depend on the example row, the
 *     stored row and d alone; final's bits depend on the request's examples, signs and weight plus the stored row: not on
 *     the batch, the slot or tile the request sits in, the order of its examples, the grid, the threshold or whether
 *     bound passes ran;
 *   - rows of slots with sign 0 are ignored whatever they hold;
 *   - out_scores / out_rows [R, k] as mmrag_cosine_topk_deep's: final descending, ties to the lower row,
 *     row + row_offset, (-inf, -1) padded;
 *   - out_pos / out_neg [R, k] float32, optional (NULL allowed): pos and neg of each hit (neg as defined above, before
 *     max(., 0); 0 when the request has no negative), recomputed as mmrag_rows_dot computes a dot, so they agree with
 *     the scan's to the float32 summation order (1e-4 on unit rows) and exactly on exactly representable data;
 *     out_scores stays authoritative.  out_pos_arg / out_neg_arg [R, k] int32, optional: the slot 0..15 that gave pos /
 *     neg, the lowest on equal dots, -1 for none.  Padding: 0 / -1;
 *   - exact: when n exceeds the candidate slots of a request (32 k, at least 16384) a sampled lower bound on the k-th
 *     final is staged first (the k-th best of any subset of live rows is at most the true k-th, whatever the score
 *     function), and only finals at or above it are kept;
 *   - at most one stream synchronisation per call, and only when n exceeds the candidate slots.
 *
 *   examples        dev [16 R, ld] of the rows' dtype and ld, pad columns zero: request g owns rows 16 g .. 16 g + 15
 *   sign            dev int8 [16 R], 4-byte aligned, values in {-1, 0, 1}
 *   neg_weight      dev float32 [R], finite, >= 0
 *   rows            dev [n, ld], MMRAG_F32 / F16 / BF16, ld of whole 128-byte slabs; MMRAG_F8E4M3 returns
 *                   MMRAG_EUNSUPPORTED (an FP8 collection is searched by examples on its re-scoring plane)
 *   k               1..MMRAG_MAX_K_DEEP
 *   alive_bits      dev, optional (NULL = every row): bit r & 31 of word r >> 5
 *   workspace       dev, >= mmrag_recommend_topk_workspace_bytes(R, n, k) bytes (0 for arguments out of range), 16-byte
 *                   aligned; short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer (the optional ones aside), R < 1 or > 2^20, n < 0 or >= 2^31,
 * k out of range, d <= 0, ld < d or not whole slabs.  sign and neg_weight live on the device and are not read by the host (the
 * Python wrapper checks the host copies it uploads). */
#define MMRAG_MAX_RECOMMEND_EXAMPLES 16
size_t mmrag_recommend_topk_workspace_bytes(int R, int64_t n, int k);
int mmrag_recommend_topk(const void *examples, const int8_t *sign, const float *neg_weight, const void *rows, int R,
                         int64_t n, int d, int64_t ld, int dtype, int k, int64_t row_offset, const uint32_t *alive_bits,
                         float *out_scores, int64_t *out_rows, float *out_pos, float *out_neg, int32_t *out_pos_arg,
                         int32_t *out_neg_arg, void *workspace, size_t workspace_bytes, void *stream);

/* Related groups (csrc/related.hip): S sets of vectors against every stored group (document) in ONE exact scan -- which
 * documents are like this set, and how much of it do they contain.  VectorIndex.related_search.
 *
 * Set s owns the columns a in set_off[s] .. set_off[s + 1]) of set_rows.  With
 *   dot[a][r]         the pair-tile body's float32 accumulation (one fixed K order: the bits equal mmrag_scoped_topk's for
 *                     the same two rows),
 *   candidate rows    r < n, alive bit set (when alive_bits is given), 0 <= group_of_row[r] < n_groups,
 *   best[a][g]        = max of dot[a][r] over the candidate rows of g, -0 read as +0,
 *   best_row[a][g]    = the LOWEST candidate row of g that attains it,
 *   similarity[s][g]  = the float64 sum of best[a][g] over the set's columns in ascending a, divided by the set's size,
 *                       rounded once to float32,
 *   covered[s][g]     = the number of the set's columns with best[a][g] >= threshold (a float32 compare),
 * the candidate groups of set s are the groups with at least one candidate row, exclude_group[s] aside, and the
 * winners are the k candidate groups of highest similarity, descending, ties to the lower ordinal.
 * Contract
 *   - out_similarity / out_group / out_covered [S, k]: the winners, (-inf, -1, 0) padded; an empty set gives padding only;
 *   - out_best / out_best_row [M, k]: for column a of set s, best[a][g] and best_row[a][g] of winner j of s,
 *     (-inf, -1) padded;
 *   - every output is a pure function of the inputs: not of the grid, the batch, or the order atomics arrive in (the
 *     scan reduces with an integer maximum of (score, lowest row) keys);
 *   - a 128-row tile of stored rows with no candidate row is not fetched;
 *   - no host synchronisation.
 *
 *   set_rows        dev [M, ld] of the rows' dtype and ld, pad columns zero; M in 0..8192
 *   set_off         dev [S + 1] int32 ascending offsets from 0 to M; S in 1..64.  Offsets that do not ascend inside
 *                   0..M own no column
 *   rows            dev [n, ld], MMRAG_F32 / F16 / BF16, ld of whole 128-byte slabs; MMRAG_F8E4M3 returns
 *                   MMRAG_EUNSUPPORTED (an FP8 collection is compared on its re-scoring plane)
 *   alive_bits      dev, optional (NULL = every row): bit r & 31 of word r >> 5
 *   group_of_row    dev [n] int32 ordinals; values outside 0..n_groups-1 are rows of no group
 *   exclude_group   dev [S] int32, -1 = none
 *   k               1..MMRAG_MAX_K_DEEP
 *   workspace       dev, >= mmrag_related_groups_workspace_bytes(M, S, n, n_groups, k) bytes (0 for arguments out of
 *                   range; it holds the 8 * M * n_groups byte table of keys), 16-byte aligned
 * MMRAG_EINVAL before anything is launched: a null pointer, M < 0 or > 8192, S < 1 or > 64, n < 0 or >= 2^31, k out of
 * range, d <= 0, ld < d or not whole slabs, n_groups < 0, a threshold that is not a number, a workspace that is too
 * small. */
#define MMRAG_MAX_RELATED_ROWS 8192
#define MMRAG_MAX_RELATED_SETS 64
size_t mmrag_related_groups_workspace_bytes(int M, int S, int64_t n, int n_groups, int k);
int mmrag_related_groups(const void *set_rows, int M, const int32_t *set_off, int S, const void *rows, int64_t n, int d,
                         int64_t ld, int dtype, const uint32_t *alive_bits, const int32_t *group_of_row, int n_groups,
                         const int32_t *exclude_group, float threshold, int k, float *out_similarity, int32_t *out_group,
                         int32_t *out_covered, float *out_best, int64_t *out_best_row, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Filtered retrieval (csrc/filtered.hip): metadata filters evaluated on the device into row bitmaps, and a batch of
 * queries answered in ONE masked scan, each query seeing only the rows of its own filter's bitmap.
 * VectorIndex.filtered_search; the filter compiler is multimodal_rag_amd/filters.py.
 *
 * A bitmap of n rows holds W = mmrag_filter_words(n) = 4 * ceil(n / 128) words (a 128-row tile is one 16-byte group):
 * bit r & 31 of word r >> 5 is row r.
 *
 * Program.  A filter is a postfix program over a boolean stack of at most 32 entries; every row runs the same
 * instructions on its own column values.  A column is MMRAG_FILTER_NUMBER (dev float64 [n], NaN = missing) or
 * MMRAG_FILTER_STRING (dev int32 [n] ordinals into the caller's dictionary, -1 = missing, read as NaN); a row's operand
 * is its column value as a double.
 *   TRUE, FALSE          push the constant
 *   AND, OR              pop two, push the result
 *   EQ NE GT GE LT LE    push (column[row] OP value), the IEEE comparison: false against NaN, NE true
 *   IN, NIN              push whether column[row] equals any / none of set_values[set_off .. set_off + set_len),
 *                        set_len in 0..MMRAG_MAX_FILTER_SET
 * The answer is the top of the stack after the last instruction.  A program holds 1..MMRAG_MAX_FILTER_OPS instructions;
 * program f is ops[prog_off[f] .. prog_off[f + 1]).
 *
 * mmrag_filter_eval: out_bits[f][w] for F programs, ANDed with alive_bits when given; bits at and past n are zero.  A
 * pure function of its inputs.  One launch, no host synchronisation, no atomics.
 *   ops, prog_off, set_values   dev; n_ops, n_set their lengths (prog_off holds F + 1 ascending offsets)
 *   columns, kinds              HOST arrays of n_columns <= MMRAG_MAX_FILTER_COLUMNS device pointers and their kinds
 *   alive_bits                  dev, optional, at least ceil(n / 32) words
 *   out_bits                    dev [F, W]
 * MMRAG_EINVAL before the launch: a null pointer, F < 1, n_ops < 1, n outside 0..2^31-1, n_columns out of range, a kind
 * that is neither.  The tables live on the device and are not read by the host: a program outside ops or longer than
 * MMRAG_MAX_FILTER_OPS matches nothing, a column index out of range reads as missing, a set out of range as empty (the
 * Python wrapper checks the host copies it holds).
 *
 * mmrag_filtered_topk: query b sees row r iff r < n and bit r of vis_bits[filter_of_query[b]] is set (the bitmaps may
 * come from mmrag_filter_eval or from anywhere else; bits at and past n are ignored).
 * Contract
 *   - out_scores / out_rows [B, k] as mmrag_cosine_topk_deep's: score descending, ties to the lower row,
 *     row + row_offset, (-inf, -1) padded;
 *   - a score's bits depend on the query row, the stored row and d alone (the pair-tile body's fixed K order) and equal
 *     mmrag_scoped_topk's for the same two rows: not on the batch, the filters, the grid or whether bound passes ran;
 *   - a 128-row tile in which no query of a 128-query tile sees a row is not fetched for that query tile;
 *   - exact under ANY bitmap: when n exceeds the candidate slots of a query (32 k, at least 16384) a sampled lower bound
 *     on each query's k-th score is staged first, from the VISIBLE rows of a strided sample of whole tiles (the k-th
 *     best of any subset of a query's visible rows is at most its true k-th), and only scores at or above it are kept;
 *   - at most one stream synchronisation per call, and only when n exceeds the candidate slots.
 *   q, rows          as mmrag_scoped_topk's; MMRAG_F8E4M3 returns MMRAG_EUNSUPPORTED
 *   k                1..MMRAG_MAX_K_DEEP
 *   filter_of_query  dev [B] int32 in 0..F-1 (anything else sees nothing; the Python wrapper checks its host copy)
 *   vis_bits         dev [F, W]
 *   workspace        dev, >= mmrag_filtered_topk_workspace_bytes(B, n, k) bytes (0 for arguments out of range), 16-byte
 *                    aligned; short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer, B < 1, F < 1, n < 0 or >= 2^31, k out of range, d <= 0,
 * ld < d or not whole slabs. */
#define MMRAG_MAX_FILTER_OPS 32
#define MMRAG_MAX_FILTER_SET 64
#define MMRAG_MAX_FILTER_COLUMNS 16
#define MMRAG_FILTER_NUMBER 0
#define MMRAG_FILTER_STRING 1
enum {
    MMRAG_FILTER_TRUE = 0, MMRAG_FILTER_FALSE, MMRAG_FILTER_AND, MMRAG_FILTER_OR, MMRAG_FILTER_EQ, MMRAG_FILTER_NE,
    MMRAG_FILTER_GT, MMRAG_FILTER_GE, MMRAG_FILTER_LT, MMRAG_FILTER_LE, MMRAG_FILTER_IN, MMRAG_FILTER_NIN
};
typedef struct {
    int32_t code, column, set_off, set_len;
    double value;
} mmrag_filter_op; /* 24 bytes */
int64_t mmrag_filter_words(int64_t n);
int mmrag_filter_eval(const mmrag_filter_op *ops, int n_ops, const int32_t *prog_off, int F, const double *set_values,
                      int n_set, const void *const *columns, const int32_t *kinds, int n_columns, int64_t n,
                      const uint32_t *alive_bits, uint32_t *out_bits, void *stream);
size_t mmrag_filtered_topk_workspace_bytes(int B, int64_t n, int k);
int mmrag_filtered_topk(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype, int k,
                        int64_t row_offset, const int32_t *filter_of_query, int F, const uint32_t *vis_bits,
                        float *out_scores, int64_t *out_rows, void *workspace, size_t workspace_bytes, void *stream);

/* Range retrieval (csrc/range.hip): not "the best k" but "everything at or above a score": how many rows pass, how they
 * spread over the values of metadata columns, and the `limit` best of them, in ONE exact masked scan (the scan of
 * mmrag_filtered_topk with another epilogue; the [B, n] score matrix is never written).  VectorIndex.range_search.
 *
 * Definitions
 *   - score(b, r) is the float32 accumulator of the pair-tile body for query row b and stored row r: the bits of
 *     mmrag_filtered_topk / mmrag_scoped_topk, a function of the two rows and d alone.
 *   - row r PASSES for query b iff r < n, r is visible to b (vis_bits == NULL: every row below n; else bit r of
 *     vis_bits[filter_of_query[b]] is set, bits at and past n ignored, a filter outside 0..F-1 sees nothing) and
 *     score(b, r) >= threshold[b].
 *   - out_count[b] = the number of passing rows.
 *   - out_facets[b], for column c at offset sum over c' < c of (G_c' + 1): slot g < G_c = the passing rows with
 *     facet_cols[c][r] == g; slot G_c = the passing rows whose code is outside 0..G_c-1 (the -1 of a row without the
 *     key).  Every column's slots sum to out_count[b].
 *   - out_scores / out_rows [B, limit] = the `limit` best passing rows: score descending, ties to the lower row,
 *     row + row_offset, (-inf, -1) padded (mmrag_cosine_topk_deep's order).
 *   - n == 0: zero counts, zero facets, padded hits.
 * Contract
 *   - counts and facets are integers added by atomics in the full pass alone: they do not depend on the batch, the
 *     grid, the order of arrival, `limit`, or whether bound passes or an overflow re-run ran;
 *   - hits are exact under any bitmap and threshold: when n exceeds the candidate slots of a query (32 limit, at least
 *     16384) a lower bound max(threshold[b], the limit-th best visible sampled score) is staged first, as
 *     mmrag_filtered_topk does, and only the candidate appends use it;
 *   - limit == 0: one pass, no select, no stream synchronisation whatever n is; limit > 0: at most one, and only when
 *     n exceeds the candidate slots;
 *   - out_count and out_facets are zeroed on `stream` by the call.
 *   q, rows          as mmrag_filtered_topk's; MMRAG_F8E4M3 returns MMRAG_EUNSUPPORTED
 *   threshold        dev [B] float32, finite (not read by the host; the Python wrapper checks its copy)
 *   limit            0..MMRAG_MAX_K_DEEP; 0 = counts and facets only, out_scores / out_rows may be NULL
 *   filter_of_query, F, vis_bits   as mmrag_filtered_topk's; vis_bits == NULL: no bitmaps, the other two are ignored
 *   facet_cols       HOST array of n_facets device columns [n] int32;  facet_sizes: HOST [n_facets], G_c >= 0
 *   n_facets         0..MMRAG_MAX_FACET_COLUMNS
 *   out_count        dev [B];  out_facets: dev [B, sum_c (G_c + 1)], NULL iff n_facets == 0
 *   workspace        dev, >= mmrag_range_scan_workspace_bytes(B, n, limit, facet_slots) bytes (0 for arguments out of
 *                    range; facet_slots = sum_c (G_c + 1), which the size does not depend on today), 16-byte aligned;
 *                    short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer, B < 1, n < 0 or >= 2^31, limit or n_facets out of range,
 * vis_bits without filter_of_query or F < 1, a negative G_c, d <= 0, ld < d or not whole slabs. */
#define MMRAG_MAX_FACET_COLUMNS 4
size_t mmrag_range_scan_workspace_bytes(int B, int64_t n, int limit, int facet_slots);
int mmrag_range_scan(const void *q, const void *rows, int B, int64_t n, int d, int64_t ld, int dtype,
                     const float *threshold, int limit, int64_t row_offset, const int32_t *filter_of_query, int F,
                     const uint32_t *vis_bits, const int32_t *const *facet_cols, const int32_t *facet_sizes, int n_facets,
                     uint32_t *out_count, uint32_t *out_facets, float *out_scores, int64_t *out_rows, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Late-interaction re-ranking (ColBERT's MaxSim) with the bi-encoder alone.  The reference has no counterpart: its
 * EmbeddingManager.rerank_results is a placeholder (app/utils/embedder.py:834-859).  The encoder's per-token outputs are
 * kept instead of pooled; a (query, passage) pair scores the mean, over the query's tokens, of each token's best cosine
 * against the passage's tokens, and the arg-max says which passage token each query token matched.
 * multimodal_rag_amd/late.py LateInteractionScorer.
 *
 * mmrag_encoder_forward_tokens (csrc/encoder.hip): the blocks of mmrag_encoder_forward, ending in token rows instead of
 * the pooled row.
 * Contract
 *   - out_tokens row t = the last hidden state of packed token t, times `proj`^T when proj is given (ONE
 *     mmrag_linear_f16, bias-free), divided by max(||.||, 1e-12): float32 sum of squares, the epsilon and the arithmetic
 *     of the pooled path's normalise, rounded to fp16 once;
 *   - out_dim is a multiple of 64, i.e. whole 128-byte fp16 slabs, so ld = mmrag_padded_dim(out_dim, MMRAG_F16) equals
 *     out_dim for every admissible shape: the rows have no pad columns (nothing to zero);
 *   - desc.pool and desc.normalize are IGNORED; desc.arch must be MMRAG_ARCH_BERT (else MMRAG_EUNSUPPORTED);
 *   - mmrag_encoder_forward is unchanged and may share the workspace (calls are stream-ordered).
 *
 *   desc, w, ids, pos_ids, cu_seqlens, T, B, max_len   as for mmrag_encoder_forward
 *   proj        dev [out_dim, H] fp16 (a ColBERT-style checkpoint's `linear`) or NULL, then out_dim must equal H
 *   out_dim     a multiple of 64, at most 1024
 *   out_tokens  dev [T, ld] fp16, ld = mmrag_padded_dim(out_dim, MMRAG_F16) = out_dim, 16-byte aligned
 *   workspace   >= mmrag_encoder_tokens_workspace_bytes(desc, T, B, out_dim) bytes (0 for arguments out of range)
 * MMRAG_EINVAL before anything is launched: a null pointer, a bad shape, out_dim not a multiple of 64 or above 1024, a
 * NULL proj with out_dim != H.  A short workspace returns MMRAG_EWORKSPACE.
 *
 * mmrag_maxsim_scores (csrc/maxsim.hip): one workgroup per pair, the query's tokens one 128-row tile, the passage walked
 * in 128-token tiles of the rows-against-rows tile body the similarity join and the k-means assign step run.
 * Contract
 *   Sequences
 *   - Query sequence s is rows q_start[s] .. q_start[s] + q_len[s] of q_tok; passage sequences likewise in d_tok.  The
 *     starts are explicit, so a caller trims [CLS] / [SEP] by moving them.  q_tok and d_tok may be one buffer.
 *   - Pair p scores query sequence pair_q[p] against passage sequence pair_d[p]; sequences may be shared between pairs.
 *   Per pair p, i over its query tokens, j over its passage tokens
 *   - best_sim[p][i] = max over j of <q_i, d_j>: float32 accumulation of the fp16 rows in the tile body's fixed K
 *     order, so its bits depend on the two rows and dim alone;
 *   - best_idx[p][i] = the LOWEST j that attains it;
 *   - out_sum[p] = the float32 sum of best_sim[p][0 .. q_len), added in ascending i starting from 0.0f;
 *   - rows past a sequence's last token are never part of a maximum (a zero row is not a token) and slots
 *     i >= q_len of best_sim / best_idx are not written.
 *   - one launch, no workspace, no host synchronisation, no atomics (the call can be captured into a graph);
 *     identical calls give identical bits.
 *
 *   q_tok, d_tok   dev [q_rows, q_ld] and [d_rows, d_ld] fp16, pad columns zero, 16-byte aligned
 *   q_ld, d_ld     mmrag_padded_dim(dim, MMRAG_F16) or a larger width of whole 128-byte slabs
 *   dim            a multiple of 64, at most 1024
 *   q_start, q_len dev [n_q] int32      d_start, d_len  dev [n_d] int32
 *   pair_q, pair_d dev [P] int32
 *   out_sum        dev [P] float32
 *   out_best_sim   dev [P, MMRAG_MAX_LATE_QUERY_TOKENS] float32 or NULL
 *   out_best_idx   dev [P, MMRAG_MAX_LATE_QUERY_TOKENS] int32 or NULL
 * MMRAG_EINVAL before anything is launched: a null pointer (the two optional outputs aside), dim out of range,
 * ld < dim or not whole slabs, P outside 1..65535, n_q, n_d, q_rows or d_rows below 1.  The tables live on the device
 * and are not read by the host: a pair whose sequence index is outside its table, whose q_len is outside
 * 1..MMRAG_MAX_LATE_QUERY_TOKENS or d_len outside 1..MMRAG_MAX_LATE_DOC_TOKENS, or whose rows do not lie inside
 * q_rows / d_rows reads no row and gets out_sum[p] = NaN (the Python wrapper checks the host copies it uploads). */
#define MMRAG_MAX_LATE_QUERY_TOKENS 128
#define MMRAG_MAX_LATE_DOC_TOKENS 512
size_t mmrag_encoder_tokens_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B, int out_dim);
int mmrag_encoder_forward_tokens(const mmrag_encoder_desc *desc, const void *const *w, const int32_t *ids,
                                 const int32_t *pos_ids, const int32_t *cu_seqlens, int64_t T, int B, int max_len,
                                 const void *proj, int out_dim, void *out_tokens, void *workspace,
                                 size_t workspace_bytes, void *stream);
int mmrag_maxsim_scores(const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok, int64_t d_rows,
                        int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                        const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                        const int32_t *pair_d, int P, float *out_sum, float *out_best_sim, int32_t *out_best_idx,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * Token store: exact MaxSim retrieval over stored token rows (csrc/maxsim_scan.hip).  The token rows of stored items
 * stay on the device in one plane, item i owning rows item_off[i] .. item_off[i + 1]; a batch of questions is answered
 * with each question's exact MaxSim top-k over ALL items in one scan of the plane, no pooled-vector search before it.
 * multimodal_rag_amd/late_store.py, VectorIndex.late_search.
 *
 * mmrag_maxsim_topk
 * Contract
 *   Sequences
 *   - Question q is rows q_start[q] .. q_start[q] + q_len[q] of q_tok, as in mmrag_maxsim_scores.
 *   - Item i is rows item_off[i] .. item_off[i + 1] of tok (item_off ascending).  An item is a CANDIDATE iff its length
 *     is in 1..MMRAG_MAX_LATE_DOC_TOKENS and, when alive_bits is given, bit i & 31 of word i >> 5 is set.  Length 0
 *     marks "no tokens stored"; such an item never appears in an output.
 *   Per question q and candidate item, i over the question's tokens, j over the item's rows
 *   - best[q][i][item] = max over j of <q_i, d_j>: float32 accumulation of the fp16 rows in the tile body's fixed K
 *     order.  Rows outside the item never take part: a zero row is not a token and a neighbour's token is not this
 *     item's;
 *   - score[q][item] = the float32 sum of best[q][0 .. q_len) in ascending i starting from 0.0f: for every
 *     (question, item) the bits equal mmrag_maxsim_scores' out_sum of the same pair;
 *   - out_scores / out_items [Q, k]: the k candidates of highest score, descending, ties to the LOWER item,
 *     (-inf, -1) padded.
 *   Guarantees
 *   - every output is a pure function of the inputs: not of the grid, the batch, how the plane is cut into chunks or
 *     whether a bound pass ran;
 *   - the per-item maxima are reduced inside one workgroup (registers, lane shuffles, LDS): no atomics, no
 *     [Q, n_items] score matrix in memory;
 *   - exact for any n_items: when n_items exceeds a question's candidate slots (32 k, at least 16384) a lower bound on
 *     its k-th score is staged first from a strided sample of whole chunks (the k-th best of any subset is at most the
 *     true k-th) and only scores at or above it are kept; a question whose survivors still overflow is produced again
 *     alone into n_items slots;
 *   - at most one stream synchronisation per call, and only when n_items exceeds the candidate slots.
 *
 *   q_tok            dev [q_rows, q_ld] fp16, pad columns zero, 16-byte aligned
 *   q_start, q_len   dev [Q] int32, lengths 1..MMRAG_MAX_LATE_QUERY_TOKENS; Q in 1..MMRAG_MAX_LATE_QUESTIONS
 *   tok              dev [T, ld] fp16, 16-byte aligned, T < 2^31
 *   q_ld, ld         mmrag_padded_dim(dim, MMRAG_F16) or a larger width of whole 128-byte slabs
 *   item_off         dev [n_items + 1] int32, ascending, inside 0..T
 *   alive_bits       dev, optional, at least ceil(n_items / 32) words (the index's alive bitmap or any `where` bitmap)
 *   dim              a multiple of 64, at most 1024
 *   k                1..MMRAG_MAX_K_DEEP
 *   out_scores       dev [Q, k] float32        out_items  dev [Q, k] int64
 *   workspace        dev, >= mmrag_maxsim_topk_workspace_bytes(Q, n_items, k) bytes (0 for arguments out of range),
 *                    16-byte aligned; short or misaligned: MMRAG_EWORKSPACE
 * MMRAG_EINVAL before anything is launched: a null pointer (alive_bits aside), Q out of range, n_items < 0 or >= 2^31,
 * T < 0 or >= 2^31, q_rows < 1, k out of range, dim out of range, ld < dim or not whole slabs.  n_items == 0 or T == 0
 * gives padding only.  The tables live on the device and are not read by the host: a question whose length is out of
 * range or whose rows do not lie inside q_rows gets padding only; an item whose rows do not lie inside the plane is no
 * candidate. */
#define MMRAG_MAX_LATE_QUESTIONS 4096
size_t mmrag_maxsim_topk_workspace_bytes(int Q, int64_t n_items, int k);
int mmrag_maxsim_topk(const void *q_tok, int64_t q_rows, int64_t q_ld, const int32_t *q_start, const int32_t *q_len,
                      int Q, const void *tok, int64_t T, int64_t ld, const int32_t *item_off, int64_t n_items,
                      const uint32_t *alive_bits, int dim, int k, float *out_scores, int64_t *out_items,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * FP8 token rows: the token store at one byte per element, MaxSim on the block-scaled FP8 matrix instruction
 * (v_mfma_scale_f32_16x16x128_f8f6f4, E4M3 x E4M3, scales 1.0).  TokenStore(dtype="float8_e4m3fn").
 *
 * Definition
 *   - An FP8 token row is a row of MMRAG_F8E4M3 codes as stored by FP8 collections: the OCP E4M3 code of x * 256
 *     rounded to nearest even, subnormals kept, magnitudes above 448 saturate to 448, NaN stores +0; pad columns are
 *     code 0.  The row pitch is mmrag_padded_dim(dim, MMRAG_F8E4M3) or a larger width of whole 128-byte slabs.
 *   - BOTH operands are code rows, the questions included (there is no mixed-precision matrix instruction): the caller
 *     quantises the question's fp16 rows first, with mmrag_f8_encode_rows.
 *   - sim(q_i, d_j) = the float32 accumulator of the decoded values' dot product in the tile body's fixed K order,
 *     times 2^-16 (exact).  The scores are the quantised rows' own; nothing is re-scored at a higher precision.
 *   - Everything else is mmrag_maxsim_scores' and mmrag_maxsim_topk's contract word for word: maxima over the item's
 *     or passage's own rows only, masked by index; best_idx the LOWEST j; the sum in ascending i from 0.0f; top-k
 *     descending, ties to the lower item, (-inf, -1) padding; every output a pure function of the inputs; the scan's
 *     score of a (question, item) has the bits of mmrag_maxsim_scores_f8's out_sum of the same pair.
 *
 * mmrag_f8_encode_rows   dst[r, c] = the code of src[r, c] for c < d, code 0 for d <= c < dst_ld.
 *   src        dev [m, src_ld] of src_dtype MMRAG_F16 or MMRAG_F32 (any other: MMRAG_EINVAL), src_ld >= d
 *   dst        dev [m, dst_ld] bytes, 16-byte aligned, dst_ld >= d of whole 128-byte slabs
 * mmrag_maxsim_scores_f8 / mmrag_maxsim_topk_f8   the arguments of mmrag_maxsim_scores / mmrag_maxsim_topk with code
 *   rows for q_tok, d_tok and tok and the FP8 pitch rule for q_ld, d_ld and ld; the same refusals, reported under
 *   their own names.  mmrag_maxsim_topk_f8_workspace_bytes is the FP8 scan's bound (its packed question tiles are
 *   half the fp16 scan's). */
int mmrag_f8_encode_rows(const void *src, int src_dtype, int64_t m, int d, int64_t src_ld, void *dst, int64_t dst_ld,
                         void *stream);
int mmrag_maxsim_scores_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const void *d_codes, int64_t d_rows,
                           int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                           const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                           const int32_t *pair_d, int P, float *out_sum, float *out_best_sim, int32_t *out_best_idx,
                           void *stream);
size_t mmrag_maxsim_topk_f8_workspace_bytes(int Q, int64_t n_items, int k);
int mmrag_maxsim_topk_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const int32_t *q_start,
                         const int32_t *q_len, int Q, const void *codes, int64_t T, int64_t ld,
                         const int32_t *item_off, int64_t n_items, const uint32_t *alive_bits, int dim, int k,
                         float *out_scores, int64_t *out_items, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Answer passages: windowed MaxSim (csrc/maxsim_windows.hip).  For a (question, passage) pair: which contiguous window
 * of the passage has the highest MaxSim against the question, and how much of the whole passage's score it keeps.
 * LateInteractionScorer.best_passages, EmbeddingManager.extract_passages, POST /query "passages".
 *
 * mmrag_maxsim_windows
 * Contract
 *   A pair p = (question sequence, passage sequence) as in mmrag_maxsim_scores; i over the question's q_len tokens,
 *   j over the passage's d_len tokens; S[i][j] = <q_i, d_j>, the tile body's float32 accumulator: the bits of
 *   mmrag_maxsim_scores' candidates.
 *   Blocks
 *   - Block g of the passage is tokens 16 g .. min(16 g + 16, d_len) (MMRAG_LATE_WINDOW_TOKENS); nb = ceil(d_len / 16),
 *     at most MMRAG_MAX_LATE_WINDOWS.  bm[i][g] = max over j in block g of S[i][j].  Columns j >= d_len are excluded
 *     by index (-inf), never by value: a zero row is not a token and a neighbour's token in the same buffer is not
 *     this passage's.
 *   Windows, given window_blocks = w in 1..MMRAG_MAX_LATE_WINDOWS
 *   - Window s covers blocks s .. min(s + w, nb) - 1, for s = 0 .. max(nb - w, 0).
 *   - win[s] = the float32 sum, in ascending i starting from 0.0f, of max over g in window s of bm[i][g].
 *   Outputs per pair
 *   - out_sum[p]       exactly mmrag_maxsim_scores' out_sum, same bits;
 *   - out_win[p][s]    win[s] for the valid s, -inf in the other slots of the MMRAG_MAX_LATE_WINDOWS;
 *   - out_best[p][3]   (start, first, last): start = the LOWEST s that attains the largest win; first, last = the
 *     tight span inside that window: for each i the lowest block g of the window with bm[i][g] equal to the window's
 *     maximum for i, first the minimum over i and last the maximum.
 *   - When w >= nb there is one window and out_win[p][0] has the bits of out_sum[p].
 *   Guarantees
 *   - one launch, no workspace, no atomics, no host synchronisation (the call can be captured into a graph);
 *   - every output is a pure function of the two sequences, dim and w.
 *
 *   q_tok .. pair_d, P   as for mmrag_maxsim_scores
 *   window_blocks        1..MMRAG_MAX_LATE_WINDOWS
 *   out_sum              dev [P] float32
 *   out_win              dev [P, MMRAG_MAX_LATE_WINDOWS] float32
 *   out_best             dev [P, 3] int32
 * MMRAG_EINVAL before anything is launched: mmrag_maxsim_scores' refusals, window_blocks out of range, a null output.
 * A pair whose table entries are out of range (mmrag_maxsim_scores' rule) reads no row and gets out_sum[p] = NaN and
 * out_best[p] = (-1, -1, -1); its out_win row is not written.  Other pairs are unaffected.
 *
 * mmrag_maxsim_windows_f8   the same over E4M3 code rows on both sides, mmrag_maxsim_scores_f8's rule word for word:
 *   maxima are compared in the accumulator domain and values are scaled, exactly, by 2^-16 where they leave;
 *   out_sum has the bits of mmrag_maxsim_scores_f8's. */
#define MMRAG_LATE_WINDOW_TOKENS 16
#define MMRAG_MAX_LATE_WINDOWS 32
int mmrag_maxsim_windows(const void *q_tok, int64_t q_rows, int64_t q_ld, const void *d_tok, int64_t d_rows,
                         int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                         const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                         const int32_t *pair_d, int P, int window_blocks, float *out_sum, float *out_win,
                         int32_t *out_best, void *stream);
int mmrag_maxsim_windows_f8(const void *q_codes, int64_t q_rows, int64_t q_ld, const void *d_codes, int64_t d_rows,
                            int64_t d_ld, int dim, const int32_t *q_start, const int32_t *q_len, int n_q,
                            const int32_t *d_start, const int32_t *d_len, int n_d, const int32_t *pair_q,
                            const int32_t *pair_d, int P, int window_blocks, float *out_sum, float *out_win,
                            int32_t *out_best, void *stream);

/* CLIP byte-level BPE (the text tower's tokenizer, BASELINE config 4; the reference only names CLIP in config.py:106).
 * Host code, multi-threaded; equals multimodal_rag_amd/tokenizer.py:ClipBpeTokenizer, which tests pin to
 * transformers.CLIPTokenizer.  The caller passes text already NFC-normalised, whitespace-collapsed and lower-cased.
 *   mmrag_clip_bpe_create   vocabulary entries as UTF-32 strings with their ids, merges ("first second") in rank order;
 *                           NULL (see mmrag_last_error) without <|startoftext|> / <|endoftext|>
 *   mmrag_clip_bpe_encode_batch  ids [n, max_length] int32, rows [sot] ids[: max_length - 2] [eot]; lens [n] */
void *mmrag_clip_bpe_create(const uint32_t *vocab_cps, const int64_t *vocab_offsets, const int32_t *vocab_ids,
                            int n_vocab, const uint32_t *merge_cps, const int64_t *merge_offsets, int n_merges);
void mmrag_clip_bpe_destroy(void *tokenizer);
int mmrag_clip_bpe_encode_batch(const void *tokenizer, const uint32_t *cps, const int64_t *offsets, int n,
                                int max_length, int32_t *ids, int32_t *lens, int n_threads);

/* Image front end of the vision tower (BASELINE config 4; the reference has no image encoder):
 * CLIP's preprocessing = shortest edge -> 224 with PIL bicubic, centre crop, done on uint8.  Bit-exact with
 * Pillow's 8-bit resampler (two integer passes, 22-bit fixed-point taps).
 *   mmrag_resample_ksize / mmrag_resample_coeffs   HOST: taps of output indices [first, first+count) of an
 *       in_size -> out_size resample; bounds [count,2] = (first input index, tap count), taps [count, ksize].
 *   mmrag_resize_crop_u8   DEVICE: src [H,W,3] uint8 (row stride src_row_bytes) -> dst [out_h,out_w,3] uint8 with
 *       horizontal taps (bx,kx: per output COLUMN of the crop) then vertical taps (by,ky: per output ROW of the
 *       crop); [y_lo,y_hi) = source rows the vertical taps touch; tmp holds (y_hi-y_lo)*out_w*3 bytes.
 *       All table and image pointers are device pointers. */
int mmrag_resample_ksize(int in_size, int out_size);
int mmrag_resample_coeffs(int in_size, int out_size, int first, int count, int32_t *bounds, int32_t *taps);
int mmrag_resize_crop_u8(const uint8_t *src, int H, int W, int64_t src_row_bytes, const int32_t *bx,
                         const int32_t *kx, int ksx, const int32_t *by, const int32_t *ky, int ksy, int out_h,
                         int out_w, int y_lo, int y_hi, uint8_t *tmp, uint8_t *dst, void *stream);

/* ---------------------------------------------------------------------------------------
 * Learned sparse retrieval (SPLADE-style term expansion): a fourth kind of evidence beside dense cosine, BM25 and
 * MaxSim.  A masked-LM head turns a chunk into a sparse vector over the vocabulary, w_v = log1p(relu(max over the
 * chunk's tokens of logit_v)); vectors are stored as 8-bit impacts in the inverted index the BM25 leg builds
 * (mmrag_lexical_csr_build, the impact in the place of tf) and a query scores a row by the integer dot product of the
 * two vectors.  multimodal_rag_amd/sparse.py DeviceSparseEncoder, ImpactIndex.
 *
 * mmrag_sparse_expand_forward (csrc/encoder.hip): the blocks of mmrag_encoder_forward, then the head's transform
 * (cls.predictions.transform: dense H x H + erf GELU + LayerNorm, on mmrag_linear_f16 and mmrag_layernorm_f16), ending
 * in UN-normalised token rows.  fp16 encoder mode, MMRAG_ARCH_BERT only (else MMRAG_EUNSUPPORTED); desc.pool and
 * desc.normalize are ignored; mmrag_encoder_forward_tokens is unchanged.
 *   desc, w, ids, pos_ids, cu_seqlens, T, B, max_len   as for mmrag_encoder_forward
 *   head_w       dev [H, H] fp16 (transform.dense.weight)     head_b  dev [H] float32
 *   head_ln_g, head_ln_b   dev [H] float32 (transform.LayerNorm), eps = desc.ln_eps
 *   out_tokens   dev [T, H] fp16, 16-byte aligned; H a multiple of 64, at most 1024
 *   workspace    >= mmrag_sparse_expand_forward_workspace_bytes(desc, T, B)
 *
 * mmrag_sparse_pool (csrc/sparse_expand.hip): the vocabulary projection and the per-chunk max in one kernel.
 * Contract
 *   - pooled[c][v] = max over the rows t of chunk c of <tok_t, E_v>, chunk c owning rows cu[c] .. cu[c + 1] of tok;
 *     float32 accumulation of the fp16 rows in the tile body's fixed K order, so the bits of every entry depend on the
 *     two rows and dim alone: not on the grid, the batch, or where a chunk falls against a tile edge;
 *   - rows of a neighbouring chunk, rows past T and decoder rows past V are never part of a maximum (they are excluded
 *     by index): a chunk whose true maximum is negative comes out negative;
 *   - the only output is pooled; nothing of size T x V is written anywhere.  No workspace, no host synchronisation (the
 *     call can be captured into a graph): chunks that span several 128-row tiles are merged in `pooled` itself by an
 *     integer atomic max on the order-preserving key of the float, which does not depend on arrival order.
 *   tok         dev [T, tok_ld] fp16, pad columns zero, 16-byte aligned       T 1..2^31 - 129
 *   cu          dev [n_chunks + 1] int32 ascending; chunk lengths 1..MMRAG_MAX_SPARSE_CHUNK_TOKENS
 *   n_chunks    1..MMRAG_MAX_SPARSE_CHUNKS
 *   E           dev [V, e_ld] fp16 decoder rows, pad columns zero, 16-byte aligned     V 1..MMRAG_MAX_SPARSE_VOCAB
 *   tok_ld, e_ld  mmrag_padded_dim(dim, MMRAG_F16) or a larger width of whole 128-byte slabs
 *   dim         a multiple of 64, at most 1024
 *   pooled      dev [n_chunks, V] float32
 *   workspace   unused (mmrag_sparse_pool_workspace_bytes is 0); may be NULL
 * MMRAG_EINVAL before anything is launched: a null pointer, dim, V, n_chunks or T out of range, a bad pitch.  The table
 * lives on the device and is not read by the host: a chunk whose rows do not lie in 0..T or whose length is outside
 * 1..MMRAG_MAX_SPARSE_CHUNK_TOKENS gets a row of -inf.
 *
 * mmrag_sparse_select (same file): activation, quantisation and the top m terms of every chunk.
 *   - w = log1pf(fmaxf(pooled[c][v] + bias[v], 0)); impact = min(255, (int)rintf(w * scale));
 *   - terms whose bit is set in skip_bits are dropped (special and [unused*] ids);
 *   - kept: the m terms of highest impact >= 1, ties to the LOWER term id; out_cnt[c] of them, written as
 *     (out_terms, out_imp)[c][0 .. out_cnt[c]) in ascending term id -- a row of the forward log
 *     mmrag_lexical_csr_build takes; the slots behind them hold (-1, 0).
 *   pooled      dev [n_chunks, V] float32     bias  dev [V] float32     skip_bits  dev [ceil(V / 32)] uint32 or NULL
 *   scale       in (0, 1024]                  m     1..MMRAG_MAX_SPARSE_TERMS
 *   out_cnt     dev [n_chunks] int32          out_terms, out_imp  dev [n_chunks, m] int32
 * MMRAG_EINVAL before anything is launched: a null pointer (skip_bits aside), V, n_chunks, m or scale out of range.
 *
 * mmrag_impact_topk (csrc/sparse_score.hip): exact top-k by integer impact score over the inverted index.
 *   - the index: term t's postings (row, impact 1..255) at term_off[t] .. term_off[t + 1), sorted by row --
 *     mmrag_lexical_csr_build's output for a forward log of (term, impact) pairs, n_terms = V;
 *   - query b: DISTINCT terms q_terms[q_off[b] .. q_off[b + 1]) with impacts q_imp 1..255, at most
 *     MMRAG_MAX_SPARSE_QUERY_TERMS of them (a query with more, or with none, matches nothing; a term outside
 *     0..n_terms or an impact outside 1..255 is skipped);
 *   - score(row) = sum over the query's terms of q_imp * impact(row, term) in int32: at most 255 * 255 * 64 < 2^24,
 *     exact, order-free and converted to float32 without rounding;
 *   - rows compete when their score is above 0 and their bit is set in alive_bits (NULL: every row);
 *   - out_scores / out_rows [B, k]: the score descending, ties to the lower row, padded with (-inf, -1);
 *   - exact in every regime: when n exceeds the candidate slots a lower bound of each query's k-th score is first
 *     taken from a strided sample of 2048-row blocks and only scores at or above it are appended; a query whose
 *     survivors still overflow is scored again alone.  At most one synchronisation of `stream` per call (to read the
 *     survivor counts), none when n fits the slots.
 *   B 1..65535     k 1..MMRAG_MAX_K_DEEP     n 0..2^31 - 2050     n_terms 0..MMRAG_MAX_SPARSE_VOCAB
 *   workspace   >= mmrag_impact_topk_workspace_bytes(B, n, k) bytes (0 for arguments out of range), 16-byte aligned */
#define MMRAG_MAX_SPARSE_CHUNK_TOKENS 512
#define MMRAG_MAX_SPARSE_CHUNKS 65536
#define MMRAG_MAX_SPARSE_VOCAB 65536
#define MMRAG_MAX_SPARSE_TERMS 256
#define MMRAG_MAX_SPARSE_QUERY_TERMS 64
size_t mmrag_sparse_expand_forward_workspace_bytes(const mmrag_encoder_desc *desc, int64_t T, int B);
int mmrag_sparse_expand_forward(const mmrag_encoder_desc *desc, const void *const *w, const int32_t *ids,
                                const int32_t *pos_ids, const int32_t *cu_seqlens, int64_t T, int B, int max_len,
                                const void *head_w, const float *head_b, const float *head_ln_g,
                                const float *head_ln_b, void *out_tokens, void *workspace, size_t workspace_bytes,
                                void *stream);
size_t mmrag_sparse_pool_workspace_bytes(int64_t T, int n_chunks, int V);
int mmrag_sparse_pool(const void *tok, int64_t T, int64_t tok_ld, const int32_t *cu, int n_chunks, const void *E, int V,
                      int64_t e_ld, int dim, float *pooled, void *workspace, size_t workspace_bytes, void *stream);
int mmrag_sparse_select(const float *pooled, const float *bias, const uint32_t *skip_bits, int n_chunks, int V,
                        float scale, int m, int32_t *out_cnt, int32_t *out_terms, int32_t *out_imp, void *stream);
size_t mmrag_impact_topk_workspace_bytes(int B, int64_t n, int k);
int mmrag_impact_topk(const int64_t *term_off, const int32_t *post_row, const int32_t *post_imp, int n_terms, int64_t n,
                      const int32_t *q_off, const int32_t *q_terms, const int32_t *q_imp, int B, int k,
                      const uint32_t *alive_bits, float *out_scores, int64_t *out_rows, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Extractive selection by sentence centrality (csrc/summarize.hip): LexRank centrality over
 * the sentences of a unit (a chunk, or an answer's context), then a budgeted MMR selection.  One workgroup per unit.
 *
 * Definition, for unit u with rows x_0 .. x_{n-1} = rows[unit_start[u] .. + unit_len[u]), 1 <= n <= 128:
 *   - S_ij = <x_i, x_j>, float32 as the 128 x 128 tile body forms it; with a bias row q = bias_rows[unit_bias[u]],
 *     s_i = <x_i, q> in the same arithmetic;
 *   - W_ij = S_ij if i != j and S_ij >= edge_threshold, else 0; deg_j = sum_i W_ij; inv_j = 1 / deg_j if deg_j > 0,
 *     else 0 (an isolated sentence's mass is dropped, not redistributed);
 *   - prior b_i = 1 / n; with a bias row r_i = max(s_i, 0) and b_i = r_i / sum(r), 1 / n when sum(r) = 0;
 *   - p = b, then EXACTLY `iterations` steps of p'_i = alpha b_i + (1 - alpha) sum_j W_ij (p_j inv_j) (no convergence
 *     test); rel_i = p_i / max_j p_j;
 *   - selection: remaining = budget[u], red_i = 0; until k picks are made or no free i has cost_i <= remaining, take
 *     the free i with cost_i <= remaining of largest v_i = lambda rel_i - (1 - lambda) red_i (ties: the lower i;
 *     lambda and 1 - lambda are float32 and each product is rounded, as in mmrag_mmr_select); then remaining -= cost_i
 *     and red_j = max(red_j, max(S_ij, 0)) for every j;
 *   - every float32 sum runs over ascending index in one thread's accumulator: a unit's output bits do not depend on
 *     the batch, the grid or its place in the plane; identical calls give identical bits;
 *   - one launch, no workspace, no host synchronisation, no atomics (the call can be captured into a graph).
 *
 *   rows        dev [n_rows, ld] of `dtype` MMRAG_F32 / F16 / BF16, pad columns zero, 16-byte aligned; MMRAG_F8E4M3
 *               returns MMRAG_EUNSUPPORTED.  ld = mmrag_padded_dim(d, dtype) or a larger width of whole 128-byte slabs
 *   unit_start, unit_len, budget   dev [n_units] int32      cost  dev [n_rows] int32, >= 1 (indexed like rows)
 *   bias_rows   dev [n_bias, ld] of the same dtype and ld, with unit_bias dev [n_units] int32 (-1: no bias row for that
 *               unit); or NULL, 0, NULL
 *   edge_threshold >= 0     alpha in (0, 1]     iterations 0..MMRAG_MAX_SUMMARY_ITERATIONS     lambda in [0, 1]
 *   k           1..MMRAG_MAX_SUMMARY_SENTENCES
 *   out_pos     dev [n_units, k] int32: the position inside the unit, in pick order, -1 padded
 *   out_val     dev [n_units, k] float32: v at the pick, -inf padded
 *   out_rel     dev [n_rows] float32 or NULL: rel of every row of a valid unit; other rows are not written
 *   out_used    dev [n_units] int32: the cost spent
 * MMRAG_EINVAL before anything is launched: a null pointer, a bad shape or pitch, n_rows outside 1..2^31 - 1, n_units
 * outside 1..2^24, a parameter out of range, a bias triple given in part.  The tables live on the device and are not
 * read by the host: a unit whose entry is out of range (unit_len outside 1..128, rows outside 0..n_rows, unit_bias
 * outside -1..n_bias - 1) gets NaN in out_val[u, 0], -1 in all of out_pos[u], 0 in out_used[u], and its out_rel rows
 * are not written (mmrag_maxsim_scores' rule). */
#define MMRAG_MAX_SUMMARY_SENTENCES 128
#define MMRAG_MAX_SUMMARY_ITERATIONS 64
int mmrag_summary_select(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *unit_start,
                         const int32_t *unit_len, int n_units, const int32_t *cost, const int32_t *budget,
                         const void *bias_rows, int64_t n_bias, const int32_t *unit_bias, float edge_threshold,
                         float alpha, int iterations, float lambda, int k, int32_t *out_pos, float *out_val,
                         float *out_rel, int32_t *out_used, void *stream);

/* Semantic chunking (csrc/chunk.hip): where to cut a document's sentences into chunks -- the
 * stage parser.py:1702-1736 `_basic_chunk_text` fills with a sliding character window.  The globally optimal
 * segmentation under the size limits, by dynamic programming over the similarities at distance < 64.  One workgroup
 * per document, documents of any length.
 *
 * Definition, for document u with rows x_0 .. x_{n-1} = rows[doc_start[u] .. + doc_len[u]), n >= 1, and costs c_i =
 * cost[doc_start[u] + i] >= 1:
 *   - S_ij = <x_i, x_j>, float32 as the 128 x 128 tile body forms it (taken with i < j);
 *   - a chunk [a, b) is admissible if b - a <= W = max_sentences and (b - a == 1 or c_a + .. + c_{b-1} <= max_cost);
 *     cost sums are exact (64-bit);
 *   - gain(a, b) = sum_{a <= i < j < b} (S_ij - tau) - penalty;
 *   - best[0] = 0, best[b] = max over admissible a in [b - W, b) of best[a] + gain(a, b); prev[b] is the arg-max, ties
 *     to the lowest a;
 *   - float32 order: R_a(b) = sum_{j = a+1}^{b-1} __fsub_rn(S_aj, tau) over ascending j in one accumulator (R_a(a+1) =
 *     0); G(b-1, b) = 0, G(a, b) = G(a+1, b) + R_a(b) for descending a; candidate v = best[a] + (G(a, b) - penalty);
 *   - tau = threshold when auto_scale == 0; else per document auto_scale * (sum_{i=0}^{n-2} S_{i,i+1}) / (n - 1): the
 *     sum over ascending i in one float32 accumulator, __fdiv_rn by (float)(n - 1), __fmul_rn; 0 when n == 1;
 *   - a document's output bits do not depend on the batch, the grid or its place in the plane;
 *   - one launch, no workspace, no host synchronisation, no atomics (the call can be captured into a graph).
 *
 *   rows        dev [n_rows, ld] of `dtype` MMRAG_F32 / F16 / BF16, pad columns zero, 16-byte aligned (MMRAG_F8E4M3 is
 *               refused).  ld = mmrag_padded_dim(d, dtype) or a larger width of whole 128-byte slabs
 *   doc_start, doc_len   dev [n_docs] int32          cost  dev [n_rows] int32, >= 1 (indexed like rows)
 *   max_cost >= 1     max_sentences 1..MMRAG_MAX_CHUNK_SENTENCES     threshold finite     auto_scale, penalty finite, >= 0
 *   out_prev    dev [n_rows] int32: out_prev[doc_start + b - 1] = prev[b], a position inside the document, b = 1..n
 *   out_best    dev [n_rows] float32: out_best[doc_start + b - 1] = best[b]
 *   out_tau     dev [n_docs] float32: the tau used
 *   out_score   dev [n_docs] float32: best[n]
 * The cuts are read from the end: b = n, then b = prev[b] until 0.
 * MMRAG_EINVAL before anything is launched: a null pointer, a bad dtype, shape or pitch, FP8 rows, n_rows outside
 * 1..2^31 - 1, n_docs outside 1..2^24, a parameter out of range.  The tables live on the device and are not read by the
 * host: a document whose entry is out of range (doc_len < 1, doc_start < 0, rows past n_rows) gets NaN in out_score[u];
 * its out_tau entry and its rows of out_prev / out_best are not written (mmrag_summary_select's rule). */
#define MMRAG_MAX_CHUNK_SENTENCES 64
int mmrag_chunk_boundaries(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *doc_start,
                           const int32_t *doc_len, int n_docs, const int32_t *cost, int32_t max_cost,
                           int max_sentences, float threshold, float auto_scale, float penalty, int32_t *out_prev,
                           float *out_best, float *out_tau, float *out_score, void *stream);

/* Answer citations (csrc/attribute.hip): which source stands behind which sentence of an
 * answer -- similarity-based attribution with the bi-encoder's rows ("this source says something very close to this
 * sentence"), not entailment.  One workgroup per unit: one answer's sentences (the claims) and its evidence sentences.
 *
 * Definition, for unit u with claims x_0 .. x_{C-1} = rows[claim_start[u] .. + claim_len[u]), 1 <= C <= 128, and
 * evidence e_0 .. e_{E-1} = rows[ev_start[u] .. + ev_len[u]), 0 <= E <= 4096, evidence row j carrying the source ordinal
 * s_j = ev_source[ev_start[u] + j] (any order; an ordinal outside 0 .. n_sources - 1: the row counts for nothing):
 *   - S_ij = <x_i, e_j>, float32 as the 128 x 128 tile body forms it (one fixed K order);
 *   - M_is = max over j with s_j = s of S_ij; J_is = the lowest such j that attains it; a source without evidence in
 *     the unit has M_is = -inf, J_is = -1;
 *   - per claim the m best sources with J_is >= 0: M_is descending, ties to the lower s;
 *   - nothing is summed but S_ij and a maximum is order-free: a unit's output bits do not depend on the batch, the grid
 *     or its place in the plane; identical calls give identical bits;
 *   - one launch, no workspace, no host synchronisation, no global atomics; the LDS maxima are over packed (score,
 *     ~j) keys, so their order cannot show in the output (the call can be captured into a graph).
 *
 *   rows        dev [n_rows, ld] of `dtype` MMRAG_F32 / F16 / BF16, pad columns zero, 16-byte aligned; MMRAG_F8E4M3
 *               returns MMRAG_EUNSUPPORTED.  ld = mmrag_padded_dim(d, dtype) or a larger width of whole 128-byte slabs
 *   claim_start, claim_len, ev_start, ev_len   dev [n_units] int32 (units may share evidence rows)
 *   ev_source   dev [n_rows] int32 (indexed like rows)
 *   n_sources   1..MMRAG_MAX_ATTR_SOURCES      m  1..MMRAG_MAX_CITATIONS      max_claims  1..MMRAG_MAX_CLAIMS
 *   out_src     dev [n_units, max_claims, m] int32: the source ordinals, best first, -1 padded
 *   out_ev      dev [n_units, max_claims, m] int32: J_is, a position inside the unit's evidence, -1 padded
 *   out_score   dev [n_units, max_claims, m] float32: M_is, -inf padded
 *   out_support dev [n_units, max_claims, n_sources] float32 or NULL: all of M; claims past C are not written
 * Rows i >= C of a valid unit hold the padding values; E = 0 is valid (every entry is padding).
 * MMRAG_EINVAL before anything is launched: a null pointer, a bad dtype, shape or pitch, n_rows outside 1..2^31 - 1,
 * n_units outside 1..2^24, n_sources, m or max_claims out of range.  The tables live on the device and are not read by
 * the host: a unit whose entry is out of range (claim_len outside 1..min(128, max_claims), ev_len outside 0..4096, rows
 * outside 0..n_rows) gets NaN in out_score[u, 0, 0], -1 in all of out_src[u] / out_ev[u], and its out_support rows are
 * not written (mmrag_summary_select's rule). */
#define MMRAG_MAX_CLAIMS 128
#define MMRAG_MAX_EVIDENCE 4096
#define MMRAG_MAX_ATTR_SOURCES 64
#define MMRAG_MAX_CITATIONS 8
int mmrag_attribute(const void *rows, int64_t ld, int dtype, int d, int64_t n_rows, const int32_t *claim_start,
                    const int32_t *claim_len, const int32_t *ev_start, const int32_t *ev_len, int n_units,
                    const int32_t *ev_source, int n_sources, int m, int max_claims, int32_t *out_src, int32_t *out_ev,
                    float *out_score, float *out_support, void *stream);

/* Measured peaks for the roofline report ("a measured stream-copy bandwidth and a measured MFMA
 * micro-benchmark peak, fractions against both the vendor and the measured peaks").  Not on the product path.
 *   mmrag_device_info        CU count, maximum shader clock (MHz), HBM bytes of the current device
 *   mmrag_bench_stream_copy  one 16-byte-per-lane copy of `bytes` bytes dst <- src (time it with events: moves 2 x bytes)
 *   mmrag_bench_stream_read  read-only stream: every lane loads 16 bytes per step (non-temporal) and sums them; one
 *                            float per thread goes to `out` (dev, 8 x 256 floats per CU).  The READ peak a scan of
 *                            the corpus is measured against (half of a copy's rate is not one).
 *   mmrag_bench_stream_write write-only stream: 16-byte non-temporal stores of a constant over `bytes` bytes
 *   mmrag_bench_mfma_f16     `iters` x 4 back-to-back v_mfma_f32_32x32x16_f16 per wave, one wave per SIMD on every CU,
 *                            operands from `seed` (dev, 256 x 16 bytes of fp16 data; use random values: the clock the
 *                            chip holds depends on them); `out` dev, 256 floats per CU; *flops = work of one launch
 *   mmrag_bench_mfma_f16_16x16x32  the same output tile per wave (64 x 64) on v_mfma_f32_16x16x32_f16: 16 per step */
int mmrag_device_info(int *n_cus, int *max_clock_mhz, int64_t *hbm_bytes);
int mmrag_bench_stream_copy(void *dst, const void *src, int64_t bytes, void *stream);
int mmrag_bench_stream_read(const void *src, int64_t bytes, float *out, void *stream);
int mmrag_bench_stream_write(void *dst, int64_t bytes, void *stream);
int mmrag_bench_mfma_f16(const void *seed, float *out, int iters, int64_t *flops, void *stream);
int mmrag_bench_mfma_f16_16x16x32(const void *seed, float *out, int iters, int64_t *flops, void *stream);

/* The encoder's building blocks, exported so each kernel can be parity-tested on its own. */
int mmrag_linear_f16(const void *x, int64_t M, int K, const void *wt, int N, const float *bias, int act,
                     const void *resid, void *out, void *stream);
int mmrag_layernorm_f16(const void *x, void *out, const float *gamma, const float *beta, int64_t T, int H,
                        float eps, void *stream);
int mmrag_embed_ln_f16(const int32_t *ids, const int32_t *pos_ids, const void *tok, const void *pos,
                       const void *type0, const float *gamma, const float *beta, void *out, int64_t T,
                       int H, int vocab, int max_pos, float eps, void *stream);
int mmrag_attention_f16(const void *qkv, const int32_t *cu_seqlens, void *ctx, int B, int max_len, int H,
                        int n_heads, int causal, void *stream);
int mmrag_pool_normalize_f16(const void *x, const int32_t *cu_seqlens, const int32_t *sel, float *out,
                             int B, int H, int pool, int normalize, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MMRAG_H */
