"""Cross-encoder re-ranking: what `sentence_transformers.CrossEncoder(name).predict(pairs)` would be to the reference's
placeholder `EmbeddingManager.rerank_results` (app/utils/embedder.py:834-859, "Re-ranking not implemented yet"; its
docstring names a cross-encoder).

Each (query, passage) pair is one packed sequence [CLS] q [SEP] p [SEP] with segment ids; the forward pass is
mmrag_cross_encoder_forward() in libmmrag.so (the encoder's HIP kernels, an embedding kernel with segment ids and a
float32 classification head).  This module owns the weight table in HBM, tokenises pairs on the host and packs them.
There is no eager / CPU forward here.

Models: a BERT-family `BertForSequenceClassification` checkpoint (e.g. cross-encoder/ms-marco-MiniLM-L-6-v2) from a
user-supplied LOCAL directory (config.json + model.safetensors + vocab.txt), or random weights of a given shape.
Nothing is downloaded.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .config import settings
from .encoder import DeviceEncoder, EncoderConfig, random_bert_weights

# the shape of cross-encoder/ms-marco-MiniLM-L-6-v2 (one relevance logit)
MS_MARCO_MINILM_L6 = EncoderConfig("ms-marco-MiniLM-L-6-v2", 6, 384, 12, 1536, max_seq_length=512, pool="cls")


class DeviceCrossEncoder(DeviceEncoder):
    """BERT sequence-pair classifier resident on one GPU.  `weights` uses the HF BertModel names (without the
    `bert.` prefix) plus `pooler.dense.{weight,bias}` and `classifier.{weight,bias}`; the token-type table must have
    at least two rows.  `precision`: "fp16" or "fp32" as for DeviceEncoder (default: MMRAG_ENCODER_PRECISION); the
    pooler and classifier are float32 in both."""

    def __init__(self, cfg: EncoderConfig, weights: Dict[str, "np.ndarray | torch.Tensor"], device="cuda:0",
                 precision: Optional[str] = None, tokenizer=None, max_length: Optional[int] = None):
        super().__init__(cfg, weights, device, precision or settings.MMRAG_ENCODER_PRECISION)
        self._use_graphs = False
        as_t = (lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)))  # noqa: E731
        tt = as_t(weights["embeddings.token_type_embeddings.weight"])
        if tt.ndim != 2 or tt.shape[0] < 2:
            raise ValueError("a cross-encoder needs a token-type table of at least 2 rows")
        cls_w = as_t(weights["classifier.weight"])
        self.n_labels = int(cls_w.shape[0])
        if not 1 <= self.n_labels <= 16:
            raise ValueError(f"n_labels = {self.n_labels}: 1..16 are supported")

        def up(x, dtype):
            t = as_t(x).to(device=self.device, dtype=torch.float32 if self._f32 else dtype).contiguous()
            self._tensors.append(t)
            return t.data_ptr()

        ptrs = list(self._ptrs)
        ptrs[2] = up(tt[:2], torch.float16)           # the whole table (rows 0 and 1), not row 0 alone
        head = [(weights["pooler.dense.weight"], (cfg.hidden, cfg.hidden)), (weights["pooler.dense.bias"], (cfg.hidden,)),
                (cls_w, (self.n_labels, cfg.hidden)), (weights["classifier.bias"], (self.n_labels,))]
        for x, shape in head:
            if tuple(as_t(x).shape) != shape:
                raise ValueError(f"head weight of shape {tuple(as_t(x).shape)}, expected {shape}")
            ptrs.append(up(x, torch.float32))
        self._ptrs = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.tokenizer = tokenizer
        self.max_length = min(max_length or cfg.max_seq_length, cfg.max_pos)

    # ---------------------------------------------------------------- constructors ---------
    @classmethod
    def random_init(cls, cfg: EncoderConfig = MS_MARCO_MINILM_L6, n_labels: int = 1, seed: int = 0, device="cuda:0",
                    std: float = 0.02, precision: Optional[str] = None, tokenizer=None) -> "DeviceCrossEncoder":
        """Seeded random weights of the given shape (benchmarks; no checkpoint can be fetched here)."""
        w = random_bert_weights(cfg, seed, device, std)
        g = torch.Generator(device=torch.device(device)).manual_seed(seed + 1)
        H = cfg.hidden
        w["pooler.dense.weight"] = torch.randn((H, H), generator=g, device=device) * std
        w["pooler.dense.bias"] = torch.randn((H,), generator=g, device=device) * std
        w["classifier.weight"] = torch.randn((n_labels, H), generator=g, device=device) * std
        w["classifier.bias"] = torch.randn((n_labels,), generator=g, device=device) * std
        return cls(cfg, w, device, precision, tokenizer)

    @classmethod
    def from_local_dir(cls, path: str, device="cuda:0", precision: Optional[str] = None,
                       max_length: Optional[int] = None) -> "DeviceCrossEncoder":
        """Load a `BertForSequenceClassification` checkpoint from a local Hugging Face style directory (config.json +
        model.safetensors + vocab.txt).  Nothing is downloaded.  Other architectures (XLM-R rerankers, ...) raise
        ValueError."""
        from safetensors.numpy import load_file

        from .tokenizer import NativeWordPieceTokenizer

        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        archs = c.get("architectures") or ["BertForSequenceClassification"]
        if c.get("model_type", "bert") != "bert" or "BertForSequenceClassification" not in archs:
            raise ValueError(f"{path}: only BERT sequence-pair classifiers (BertForSequenceClassification) are "
                             f"supported, not model_type={c.get('model_type')!r} {archs}")
        if c.get("position_embedding_type", "absolute") != "absolute" or c.get("hidden_act", "gelu") != "gelu":
            raise ValueError(f"{path}: only absolute positions and erf GELU are built")
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
        id2label = c.get("id2label")
        n_labels = len(id2label) if id2label else int(c.get("num_labels", 2))
        if w["classifier.weight"].shape[0] != n_labels:
            raise ValueError(f"{path}: classifier has {w['classifier.weight'].shape[0]} rows, config {n_labels} labels")
        tok = NativeWordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"), lower)
        return cls(cfg, w, device, precision, tok, max_length or tk_max)

    # ---------------------------------------------------------------- forward ---------------
    def score_ids(self, ids, type_ids, lens=None) -> torch.Tensor:
        """Logits [B, n_labels] float32 on the device.  Either lists of token-id / type-id sequences, or (what
        `NativeWordPieceTokenizer.encode_pairs_arrays` returns) 2-D int32 arrays with `lens`."""
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
        if lens.max() > self.cfg.max_pos:
            raise ValueError(f"sequence of {int(lens.max())} tokens > max_position_embeddings {self.cfg.max_pos}")
        W = ids.shape[1]
        keep = np.arange(W, dtype=np.int32)[None, :] < lens[:, None]
        flat = [np.ascontiguousarray(ids[keep], np.int32), np.ascontiguousarray(type_ids[keep], np.int32),
                np.broadcast_to(np.arange(W, dtype=np.int32)[None, :], ids.shape)[keep]]
        cu = np.zeros(len(lens) + 1, np.int32)
        np.cumsum(lens, out=cu[1:])
        n = flat[0].size
        n4 = (n + 3) & ~3
        host = torch.empty(3 * n4 + cu.size, dtype=torch.int32)
        if self.device.type == "cuda":
            host = host.pin_memory()
        h = host.numpy()
        for j, f in enumerate(flat):
            h[j * n4: j * n4 + n] = f
        h[3 * n4:] = cu
        dev = host.to(self.device, non_blocking=True)
        d_ids, d_types, d_pos, d_cu = dev[:n], dev[n4:n4 + n], dev[2 * n4:2 * n4 + n], dev[3 * n4:]
        T, B = n, len(lens)
        need = _native.cross_encoder_workspace_bytes(self.desc, T, B, self._f32)
        with self._launch_lock:
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            return _native.cross_encoder_forward(self.desc, self._ptrs, self.n_labels, d_ids, d_types, d_pos, d_cu,
                                                 int(lens.max()), workspace=self._workspace, f32=self._f32)

    def tokenize_pairs(self, pairs: Sequence[Tuple[str, str]]):
        """(ids [n, W], type_ids [n, W], lens [n]) int32 arrays of the pairs"""
        if self.tokenizer is None:
            raise RuntimeError("this cross-encoder has no tokenizer (load it with from_local_dir or pass one)")
        firsts = [p[0] for p in pairs]
        seconds = [p[1] if p[1] is not None else "" for p in pairs]
        if hasattr(self.tokenizer, "encode_pairs_arrays"):
            return self.tokenizer.encode_pairs_arrays(firsts, seconds, self.max_length)
        rows = [self.tokenizer.encode_pair(a, b, self.max_length) for a, b in zip(firsts, seconds)]
        ids = np.zeros((len(rows), self.max_length), np.int32)
        types = np.zeros_like(ids)
        for i, (r, t) in enumerate(rows):
            ids[i, : len(r)], types[i, : len(t)] = r, t
        return ids, types, np.array([len(r) for r, _ in rows], np.int32)

    def predict(self, pairs: Sequence[Tuple[str, str]], batch_size: int = 32,
                apply_sigmoid: Optional[bool] = None) -> np.ndarray:
        """Scores of (query, passage) pairs, as `CrossEncoder.predict`: [n] for a single-label model (sigmoid applied
        unless apply_sigmoid=False), else [n, n_labels] raw logits (apply_sigmoid=True applies it there too).  A
        query shared by consecutive pairs is tokenised once per batch."""
        pairs = list(pairs)
        if apply_sigmoid is None:
            apply_sigmoid = self.n_labels == 1
        out: List[np.ndarray] = []
        for s in range(0, len(pairs), max(1, batch_size)):
            ids, types, lens = self.tokenize_pairs(pairs[s: s + batch_size])
            out.append(self.score_ids(ids, types, lens).cpu().numpy())
        logits = np.concatenate(out) if out else np.zeros((0, self.n_labels), np.float32)
        if apply_sigmoid:
            logits = (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
        return logits[:, 0] if self.n_labels == 1 else logits
