"""Extractive reader: the answer span itself ("14 March 2019", not the paragraph around it), and whether the passages
hold an answer at all -- what `transformers.pipeline("question-answering")` / a Haystack reader would be to this
service.  Not in the reference.

Each (question, passage window) pair is one packed sequence [CLS] question [SEP] window [SEP] with segment ids; the
forward pass is mmrag_reader_forward() in libmmrag.so: the encoder's HIP kernels, the embedding kernel with segment ids
and the span head (csrc/span_head.hip: start / end logits, their log-sum-exp over [CLS] and the window, and the n best
disjoint spans, one launch, nothing but the spans copied back).  This module owns the weight table in HBM, cuts long
passages into overlapping windows, packs the rows and maps token spans back to characters.  There is no eager / CPU
forward here.

Models: a BERT-family `BertForQuestionAnswering` checkpoint (e.g. a SQuAD2-trained BERT) from a user-supplied LOCAL
directory (config.json + model.safetensors + vocab.txt), or random weights of a given shape.  Nothing is downloaded.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from .encoder import DeviceEncoder, EncoderConfig, random_bert_weights
from .reranker import MS_MARCO_MINILM_L6

MAX_READER_TOKENS = _native.MAX_READER_TOKENS
MAX_ANSWER_TOKENS = _native.MAX_ANSWER_TOKENS
MAX_READER_SPANS = _native.MAX_READER_SPANS
ALL_TOKENS = 1 << 30          # "no truncation" for encode_with_spans
TOKEN_BUDGET = 16384          # packed tokens of one forward


# ---------------------------------------------------------------- host logic (no device) ---------
def cut_windows(n_tokens: int, window: int, doc_stride: int) -> List[Tuple[int, int]]:
    """(start, length) of the windows of a passage of `n_tokens` tokens: one when it fits `window`, else windows of
    `window` tokens of which consecutive ones share `doc_stride` tokens (at most half a window, so that a short window
    still advances), the last one shorter.  Every token is in a window; an empty passage has one empty window."""
    if window < 1:
        raise ValueError("window must be >= 1")
    if n_tokens <= window:
        return [(0, max(n_tokens, 0))]
    step = window - min(max(int(doc_stride), 0), window // 2)
    out, at = [], 0
    while True:
        out.append((at, min(window, n_tokens - at)))
        if at + window >= n_tokens:
            return out
        at += step


def plan_rows(tokenizer, questions: Sequence[str], passages: Sequence[str], max_length: int, doc_stride: int,
              max_query_tokens: int):
    """The rows of one read call.  Every distinct question is tokenised once (truncated to `max_query_tokens`), every
    passage once, with character spans.  Returns (rows, spans): rows[r] = {"passage", "offset" (the window's first
    token in the passage), "ids", "type_ids", "ctx_start", "ctx_len"}, the windows of a passage consecutive;
    spans[p] = the (start, end) characters of passage p's tokens."""
    if len(questions) != len(passages):
        raise ValueError(f"{len(questions)} questions for {len(passages)} passages")
    if max_length < 5 or max_length > MAX_READER_TOKENS:
        raise ValueError(f"max_length must be in 5..{MAX_READER_TOKENS}")
    cls, sep = tokenizer.cls, tokenizer.sep
    q_cache: Dict[str, List[int]] = {}
    rows, spans = [], []
    for p, (question, text) in enumerate(zip(questions, passages)):
        if question not in q_cache:
            keep = max(1, min(int(max_query_tokens), max_length - 4))
            q_cache[question] = list(tokenizer.encode_with_spans(question, keep + 2)[0][1:-1])
        q = q_cache[question]
        ids, sp = tokenizer.encode_with_spans(text if text is not None else "", ALL_TOKENS)
        ids, sp = list(ids[1:-1]), list(sp[1:-1])
        spans.append(sp)
        head = [cls] + q + [sep]
        for start, length in cut_windows(len(ids), max_length - len(q) - 3, doc_stride):
            rows.append({"passage": p, "offset": start, "ids": head + ids[start: start + length] + [sep],
                         "type_ids": [0] * len(head) + [1] * (length + 1), "ctx_start": len(head), "ctx_len": length})
    return rows, spans


def chunk_rows(lens: Sequence[int], budget: int = TOKEN_BUDGET) -> List[Tuple[int, int]]:
    """[lo, hi) runs of consecutive rows of at most `budget` tokens each (a single longer row is a run of its own)"""
    out, lo, used = [], 0, 0
    for r, n in enumerate(lens):
        if r > lo and used + n > budget:
            out.append((lo, r))
            lo, used = r, 0
        used += n
    if len(lens) > lo:
        out.append((lo, len(lens)))
    return out


def select_disjoint(cands: List[Dict[str, Any]], n_best: int) -> List[Dict[str, Any]]:
    """The kernel's selection rule over a passage's candidates from all its windows: entries with the same character
    span are one candidate (the higher score stays); then best first -- higher score, then lower first token, then lower
    last token -- skipping a candidate that shares a token with one already kept; at most `n_best`."""
    best: Dict[Tuple[int, int], Dict[str, Any]] = {}
    for c in cands:
        key = (c["start"], c["end"])
        if key not in best or (-c["score"], c["tok"]) < (-best[key]["score"], best[key]["tok"]):
            best[key] = c
    kept: List[Dict[str, Any]] = []
    for c in sorted(best.values(), key=lambda c: (-c["score"], c["tok"][0], c["tok"][1])):
        if len(kept) >= n_best:
            break
        if all(c["tok"][1] < k["tok"][0] or k["tok"][1] < c["tok"][0] for k in kept):
            kept.append(c)
    return kept


def assemble(passages: Sequence[str], rows, spans, span, score, null, lse, n_best: int) -> List[Dict[str, Any]]:
    """Per passage {"spans": [{"text", "start", "end", "score", "probability"} ...] best first, "null_score"} from the
    kernel's per-row outputs (host arrays: span [R, n, 2], score [R, n], null [R], lse [R, 2])."""
    cands: List[List[Dict[str, Any]]] = [[] for _ in passages]
    nulls: List[List[float]] = [[] for _ in passages]
    for r, row in enumerate(rows):
        p, sp = row["passage"], spans[row["passage"]]
        nulls[p].append(float(null[r]))
        for k in range(span.shape[1]):
            i, j = int(span[r, k, 0]), int(span[r, k, 1])
            if i < 0:
                continue
            ti, tj = row["offset"] + i - row["ctx_start"], row["offset"] + j - row["ctx_start"]
            s = float(score[r, k])
            cands[p].append({"start": sp[ti][0], "end": max(sp[ti][1], sp[tj][1]), "score": s, "tok": (ti, tj),
                             "probability": min(1.0, math.exp(s - float(lse[r, 0]) - float(lse[r, 1])))})
    out = []
    for p, text in enumerate(passages):
        kept = select_disjoint(cands[p], n_best)
        out.append({"spans": [{"text": (text or "")[c["start"]: c["end"]], "start": c["start"], "end": c["end"],
                               "score": c["score"], "probability": c["probability"]} for c in kept],
                    "null_score": min(nulls[p]) if nulls[p] else float("nan")})
    return out


def best_answers(read_out: Sequence[Dict[str, Any]], owner: Sequence[int], n_answers: int,
                 null_threshold: float) -> Dict[str, Any]:
    """{"answers", "answerable", "null_score"} over the passages of one question: `owner[p]` is the hit passage p
    belongs to.  answers: the best `n_answers` spans over all passages -- {"text", "score", "probability", "hit",
    "passage", "start", "end"} -- character-identical texts merged (the best stays).  answerable: best span score - lowest null
    score > null_threshold."""
    seen: Dict[str, Dict[str, Any]] = {}
    order = []
    for p, found in enumerate(read_out):
        for s in found["spans"]:
            order.append({"text": s["text"], "score": s["score"], "probability": s["probability"], "hit": owner[p],
                          "passage": p, "start": s["start"], "end": s["end"]})
    for a in sorted(order, key=lambda a: -a["score"]):      # stable: ties keep hit order
        seen.setdefault(a["text"], a)
    answers = list(seen.values())[: max(int(n_answers), 0)]
    nulls = [f["null_score"] for f in read_out if not math.isnan(f["null_score"])]
    null_score = min(nulls) if nulls else None
    answerable = bool(answers) and (null_score is None or answers[0]["score"] - null_score > null_threshold)
    return {"answers": answers, "answerable": answerable, "null_score": null_score}


# ---------------------------------------------------------------- the device model ---------
class DeviceReader(DeviceEncoder):
    """BERT question-answering model resident on one GPU.  `weights` uses the HF BertModel names (without the `bert.`
    prefix) plus `qa_outputs.{weight,bias}` ([2, hidden], [2]: row 0 start, row 1 end); the token-type table must have
    at least two rows.  fp16 mode only (the span head is float32)."""

    def __init__(self, cfg: EncoderConfig, weights: Dict[str, "np.ndarray | torch.Tensor"], device="cuda:0",
                 precision: Optional[str] = None, tokenizer=None, max_length: Optional[int] = None):
        if (precision or "fp16") != "fp16":
            raise ValueError(f"precision {precision!r}: fp16 is the only reader mode built")
        super().__init__(cfg, weights, device, "fp16")
        self._use_graphs = False
        as_t = (lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)))  # noqa: E731
        tt = as_t(weights["embeddings.token_type_embeddings.weight"])
        if tt.ndim != 2 or tt.shape[0] < 2:
            raise ValueError("a reader needs a token-type table of at least 2 rows")

        def up(x, dtype):
            t = as_t(x).to(device=self.device, dtype=dtype).contiguous()
            self._tensors.append(t)
            return t.data_ptr()

        ptrs = list(self._ptrs)
        ptrs[2] = up(tt[:2], torch.float16)           # the whole table (rows 0 and 1), not row 0 alone
        for x, shape in ((weights["qa_outputs.weight"], (2, cfg.hidden)), (weights["qa_outputs.bias"], (2,))):
            if tuple(as_t(x).shape) != shape:
                raise ValueError(f"qa_outputs weight of shape {tuple(as_t(x).shape)}, expected {shape}")
            ptrs.append(up(x, torch.float32))
        self._ptrs = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.tokenizer = tokenizer
        self.max_length = min(max_length or cfg.max_seq_length, cfg.max_pos, MAX_READER_TOKENS)

    # ---------------------------------------------------------------- constructors ---------
    @classmethod
    def random_init(cls, cfg: EncoderConfig = MS_MARCO_MINILM_L6, seed: int = 0, device="cuda:0", std: float = 0.02,
                    precision: Optional[str] = None, tokenizer=None) -> "DeviceReader":
        """Seeded random weights of the given shape (no checkpoint can be fetched here)."""
        w = random_bert_weights(cfg, seed, device, std)
        g = torch.Generator(device=torch.device(device)).manual_seed(seed + 1)
        w["qa_outputs.weight"] = torch.randn((2, cfg.hidden), generator=g, device=device) * std
        w["qa_outputs.bias"] = torch.randn((2,), generator=g, device=device) * std
        return cls(cfg, w, device, precision, tokenizer)

    @staticmethod
    def check_config(path: str, c: Dict[str, Any]) -> None:
        """ValueError unless config.json describes a BertForQuestionAnswering with absolute positions and erf GELU"""
        archs = c.get("architectures") or []
        if c.get("model_type") != "bert" or "BertForQuestionAnswering" not in archs:
            raise ValueError(f"{path}: only BERT extractive readers (BertForQuestionAnswering) are supported, not "
                             f"model_type={c.get('model_type')!r} {archs}")
        if c.get("position_embedding_type", "absolute") != "absolute" or c.get("hidden_act", "gelu") != "gelu":
            raise ValueError(f"{path}: only absolute positions and erf GELU are built")

    @classmethod
    def from_local_dir(cls, path: str, device="cuda:0", precision: Optional[str] = None,
                       max_length: Optional[int] = None) -> "DeviceReader":
        """Load a `BertForQuestionAnswering` checkpoint from a local Hugging Face style directory (config.json +
        model.safetensors + vocab.txt).  Nothing is downloaded.  Other architectures raise ValueError."""
        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        cls.check_config(path, c)
        if (precision or "fp16") != "fp16":
            raise ValueError(f"precision {precision!r}: fp16 is the only reader mode built")
        from safetensors.numpy import load_file

        from .tokenizer import NativeWordPieceTokenizer

        lower, tk_max = True, None
        tk_cfg = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(tk_cfg):
            with open(tk_cfg) as f:
                t = json.load(f)
            lower = t.get("do_lower_case", True)
            m = t.get("model_max_length")
            tk_max = int(m) if isinstance(m, (int, float)) and m < 1e6 else None
        cfg = EncoderConfig(os.path.basename(os.path.normpath(path)), c["num_hidden_layers"], c["hidden_size"],
                            c["num_attention_heads"], c["intermediate_size"], c["vocab_size"],
                            c["max_position_embeddings"], c["max_position_embeddings"], "cls",
                            c.get("layer_norm_eps", 1e-12))
        raw = load_file(os.path.join(path, "model.safetensors"))
        w = {(k[5:] if k.startswith("bert.") else k): v for k, v in raw.items()}
        for k in ("qa_outputs.weight", "qa_outputs.bias"):
            if k not in w:
                raise ValueError(f"{path}: model.safetensors has no {k}")
        tok = NativeWordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"), lower)
        return cls(cfg, w, device, precision, tok, max_length or tk_max)

    # ---------------------------------------------------------------- forward ---------------
    def read_ids(self, ids, type_ids, lens, ctx_start, ctx_len, max_answer_tokens: int = 30, n_best: int = 3,
                 logits: bool = False):
        """(spans [B, n_best, 2] int32, scores [B, n_best], null [B], lse [B, 2], logits [T, 2] or None) on the device
        for packed rows: lists of token-id / type-id sequences (`lens` None) or 2-D int32 arrays with `lens`;
        `ctx_start` / `ctx_len` [B]: the passage's tokens inside each row."""
        if lens is None:
            W = max((len(s) for s in ids), default=0)
            lens = np.array([len(s) for s in ids], np.int32)
            a, t = np.zeros((len(ids), max(W, 1)), np.int32), np.zeros((len(ids), max(W, 1)), np.int32)
            for i, (s, ty) in enumerate(zip(ids, type_ids)):
                if len(ty) != len(s):
                    raise ValueError("ids and type_ids differ in length")
                a[i, : len(s)], t[i, : len(s)] = s, ty
            ids, type_ids = a, t
        lens = np.asarray(lens, np.int32)
        if lens.size == 0 or lens.min() <= 0:
            raise ValueError("empty token sequence")
        if lens.max() > min(self.cfg.max_pos, MAX_READER_TOKENS):
            raise ValueError(f"sequence of {int(lens.max())} tokens > {min(self.cfg.max_pos, MAX_READER_TOKENS)}")
        B = len(lens)
        cs, cl = np.asarray(ctx_start, np.int32).reshape(-1), np.asarray(ctx_len, np.int32).reshape(-1)
        if cs.size != B or cl.size != B:
            raise ValueError("ctx_start / ctx_len need one entry per row")
        W = ids.shape[1]
        keep = np.arange(W, dtype=np.int32)[None, :] < lens[:, None]
        flat = [np.ascontiguousarray(ids[keep], np.int32), np.ascontiguousarray(type_ids[keep], np.int32),
                np.broadcast_to(np.arange(W, dtype=np.int32)[None, :], ids.shape)[keep]]
        cu = np.zeros(B + 1, np.int32)
        np.cumsum(lens, out=cu[1:])
        n = flat[0].size
        n4, b4 = (n + 3) & ~3, (B + 4) & ~3
        host = torch.empty(3 * n4 + 3 * b4, dtype=torch.int32)
        if self.device.type == "cuda":
            host = host.pin_memory()
        h = host.numpy()
        for j, f in enumerate(flat):
            h[j * n4: j * n4 + n] = f
        h[3 * n4: 3 * n4 + B + 1] = cu
        h[3 * n4 + b4: 3 * n4 + b4 + B] = cs
        h[3 * n4 + 2 * b4: 3 * n4 + 2 * b4 + B] = cl
        dev = host.to(self.device, non_blocking=True)
        d_ids, d_types, d_pos = dev[:n], dev[n4:n4 + n], dev[2 * n4:2 * n4 + n]
        d_cu, d_cs, d_cl = dev[3 * n4: 3 * n4 + B + 1], dev[3 * n4 + b4: 3 * n4 + b4 + B], \
            dev[3 * n4 + 2 * b4: 3 * n4 + 2 * b4 + B]
        need = _native.reader_workspace_bytes(self.desc, n, B)
        with self._launch_lock:
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            return _native.reader_forward(self.desc, self._ptrs, d_ids, d_types, d_pos, d_cu, d_cs, d_cl,
                                          int(lens.max()), max_answer_tokens, n_best, logits, self._workspace)

    def read(self, question: Union[str, Sequence[str]], passages: Sequence[str], n_best: int = 3,
             max_answer_tokens: int = 30, doc_stride: int = 128, max_query_tokens: int = 64,
             details: bool = False):
        """The `n_best` disjoint answer spans of every passage: per passage {"spans": [{"text", "start", "end", "score",
        "probability"} ...] best first, "null_score"}; text == passage[start:end].  `question`: one for all passages,
        or one per passage.  A passage that does not fit next to the question is cut into windows of max_length -
        |question| - 3 tokens that share `doc_stride` tokens; its windows' spans are merged (select_disjoint) and its
        null_score is the lowest of its windows (the SQuAD2 convention).  score = start logit + end logit;
        probability = exp(score - lse_start - lse_end) of the window the span came from.  One forward for all rows,
        in runs of TOKEN_BUDGET tokens.  `details`: also return (rows, kernel outputs on the host) for inspection."""
        if self.tokenizer is None:
            raise RuntimeError("this reader has no tokenizer (load it with from_local_dir or pass one)")
        if not 1 <= n_best <= MAX_READER_SPANS:
            raise ValueError(f"n_best must be in 1..{MAX_READER_SPANS}")
        if not 1 <= max_answer_tokens <= MAX_ANSWER_TOKENS:
            raise ValueError(f"max_answer_tokens must be in 1..{MAX_ANSWER_TOKENS}")
        passages = list(passages)
        questions = [question] * len(passages) if isinstance(question, str) else list(question)
        rows, spans = plan_rows(self.tokenizer, questions, passages, self.max_length, doc_stride, max_query_tokens)
        outs = []
        for lo, hi in chunk_rows([len(r["ids"]) for r in rows]):
            part = rows[lo:hi]
            got = self.read_ids([r["ids"] for r in part], [r["type_ids"] for r in part], None,
                                [r["ctx_start"] for r in part], [r["ctx_len"] for r in part], max_answer_tokens, n_best)
            outs.append(got[:4])
        if outs:
            span, score, null, lse = (torch.cat([o[k] for o in outs]).cpu().numpy() for k in range(4))
        else:
            span, score = np.zeros((0, n_best, 2), np.int32), np.zeros((0, n_best), np.float32)
            null, lse = np.zeros(0, np.float32), np.zeros((0, 2), np.float32)
        out = assemble(passages, rows, spans, span, score, null, lse, n_best)
        return (out, rows, (span, score, null, lse)) if details else out
