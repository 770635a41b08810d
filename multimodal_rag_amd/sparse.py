"""Learned sparse retrieval (SPLADE-style term expansion): the fourth kind of evidence beside dense cosine, BM25 and
MaxSim.

A masked-LM head turns a text into a sparse vector over the vocabulary, w_v = log1p(relu(max over the text's tokens of
logit_v)): the encoder supplies expansion terms ("car" gives weight to "automobile"), the index stays inverted and the
scores exact and explainable.  Everything that computes is in libmmrag.so:

    mmrag_sparse_expand_forward   encoder layers + cls.predictions.transform -> un-normalised token rows
    mmrag_sparse_pool             vocabulary projection and per-text max in ONE kernel: the [T, V] logits never exist
    mmrag_sparse_select           log1p(relu(.)), 8-bit impacts, the top m terms of each text in ascending term id
    mmrag_lexical_csr_build       the BM25 leg's inverted-index build, the impact in the place of tf
    mmrag_impact_topk             exact integer scoring and top-k over that index

This module owns the weights in HBM (`DeviceSparseEncoder`) and the device state of one collection (`ImpactIndex`,
shaped like `lexical.LexicalIndex`).  Models: a `BertForMaskedLM` checkpoint (e.g. a SPLADE checkpoint) from a
user-supplied LOCAL directory, or random weights of a given shape.  Nothing is downloaded; there is no eager forward.
"""
from __future__ import annotations

import ctypes
import json
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .encoder import DeviceEncoder, EncoderConfig, random_bert_weights

HEAD_KEYS = ("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias",
             "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias",
             "cls.predictions.bias")
DECODER_KEY = "cls.predictions.decoder.weight"
TIED_KEY = "embeddings.word_embeddings.weight"
_SPECIAL = re.compile(r"^\[(PAD|UNK|CLS|SEP|MASK|unused\d+)\]$")


def load_sparse_checkpoint(path: str, max_seq_length: Optional[int] = None):
    """(EncoderConfig, weights, lower-casing flag) of a local `BertForMaskedLM` directory (config.json +
    model.safetensors): HF BertModel names without the `bert.` prefix plus the `cls.predictions.*` head;
    `cls.predictions.decoder.weight` falls back to the tied word embeddings when the file omits it.  Host only.
    Other architectures raise ValueError."""
    from safetensors.numpy import load_file

    with open(os.path.join(path, "config.json")) as f:
        c = json.load(f)
    archs = c.get("architectures") or ["BertForMaskedLM"]
    if c.get("model_type", "bert") != "bert" or "BertForMaskedLM" not in archs:
        raise ValueError(f"{path}: only BERT masked-LM checkpoints (BertForMaskedLM) are supported, not "
                         f"model_type={c.get('model_type')!r} {archs}")
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
    max_len = min(max_seq_length or tk_max or c["max_position_embeddings"], c["max_position_embeddings"])
    cfg = EncoderConfig(os.path.basename(os.path.normpath(path)), c["num_hidden_layers"], c["hidden_size"],
                        c["num_attention_heads"], c["intermediate_size"], c["vocab_size"],
                        c["max_position_embeddings"], max_len, "cls", c.get("layer_norm_eps", 1e-12))
    raw = load_file(os.path.join(path, "model.safetensors"))
    w = {(k[5:] if k.startswith("bert.") else k): v for k, v in raw.items()}
    missing = [k for k in HEAD_KEYS if k not in w]
    if missing:
        raise ValueError(f"{path}: the masked-LM head is incomplete, missing {missing}")
    if DECODER_KEY not in w:
        w[DECODER_KEY] = w[TIED_KEY]            # tie_word_embeddings: the decoder is the embedding table
    return cfg, w, lower


def skip_ids_of_vocab(vocab: Dict[str, int]) -> np.ndarray:
    """ids that never become terms: [PAD] [UNK] [CLS] [SEP] [MASK] and the [unused*] slots"""
    return np.asarray(sorted(i for t, i in vocab.items() if _SPECIAL.match(t)), np.int64)


class DeviceSparseEncoder(DeviceEncoder):
    """BERT masked-LM resident on one GPU, used as a term expander.  `weights`: the HF BertModel names plus
    `cls.predictions.transform.dense.{weight,bias}`, `cls.predictions.transform.LayerNorm.{weight,bias}`,
    `cls.predictions.bias` and `cls.predictions.decoder.weight` (absent: the tied word embeddings).  fp16 mode only.
    `scale`: impacts are min(255, rint(w * scale)) (default MMRAG_SPARSE_IMPACT_SCALE)."""

    def __init__(self, cfg: EncoderConfig, weights: Dict[str, "np.ndarray | torch.Tensor"], device="cuda:0",
                 tokenizer=None, scale: Optional[float] = None, skip_ids: Optional[Sequence[int]] = None):
        from .config import settings

        if cfg.hidden % 64 or cfg.hidden > 1024:
            raise ValueError(f"hidden = {cfg.hidden}: the sparse head needs a multiple of 64, at most 1024")
        if not 1 <= cfg.vocab <= _native.MAX_SPARSE_VOCAB:
            raise ValueError(f"vocab = {cfg.vocab}: 1..{_native.MAX_SPARSE_VOCAB} are supported")
        super().__init__(cfg, weights, device, "fp16")
        as_t = (lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)))  # noqa: E731
        H, V = cfg.hidden, cfg.vocab
        dec = weights[DECODER_KEY] if DECODER_KEY in weights else weights[TIED_KEY]
        want = [(HEAD_KEYS[0], (H, H), torch.float16), (HEAD_KEYS[1], (H,), torch.float32),
                (HEAD_KEYS[2], (H,), torch.float32), (HEAD_KEYS[3], (H,), torch.float32),
                (HEAD_KEYS[4], (V,), torch.float32)]
        head = []
        for key, shape, dtype in want:
            t = as_t(weights[key])
            if tuple(t.shape) != shape:
                raise ValueError(f"{key} of shape {tuple(t.shape)}, expected {shape}")
            head.append(t.to(device=self.device, dtype=dtype).contiguous())
        dec = as_t(dec)
        if tuple(dec.shape) != (V, H):
            raise ValueError(f"decoder rows of shape {tuple(dec.shape)}, expected {(V, H)}")
        self._head_w, self._head_b, self._head_g, self._head_beta, self.vocab_bias = head
        self._decoder = dec.to(device=self.device, dtype=torch.float16).contiguous()   # [V, H]: H % 64 == 0, no pad columns
        self._tensors.extend(head + [self._decoder])
        self.tokenizer = tokenizer
        self.scale = float(settings.MMRAG_SPARSE_IMPACT_SCALE if scale is None else scale)
        if skip_ids is None and tokenizer is not None and getattr(tokenizer, "vocab", None):
            skip_ids = skip_ids_of_vocab(tokenizer.vocab)
        flags = np.zeros((V + 31) // 32 * 32, bool)
        if skip_ids is not None and len(skip_ids):
            ids = np.asarray(skip_ids, np.int64)
            flags[ids[(ids >= 0) & (ids < V)]] = True
        self._skip_host = flags[:V].copy()
        self._skip_bits = torch.from_numpy(np.packbits(flags, bitorder="little").view(np.int32).copy()).to(self.device)
        self._id2tok: Optional[List[str]] = None

    # ---------------------------------------------------------------- constructors ---------
    @classmethod
    def random_init(cls, cfg: EncoderConfig, seed: int = 0, device="cuda:0", std: float = 0.02, tokenizer=None,
                    scale: Optional[float] = None, tied: bool = True) -> "DeviceSparseEncoder":
        """Seeded random weights of the given shape (benchmarks and tests; no checkpoint can be fetched here)."""
        w = random_bert_weights(cfg, seed, device, std)
        g = torch.Generator(device=torch.device(device)).manual_seed(seed + 1)
        H, V = cfg.hidden, cfg.vocab
        w[HEAD_KEYS[0]] = torch.randn((H, H), generator=g, device=device) * std
        w[HEAD_KEYS[1]] = torch.randn((H,), generator=g, device=device) * std
        w[HEAD_KEYS[2]] = 1.0 + torch.randn((H,), generator=g, device=device) * std
        w[HEAD_KEYS[3]] = torch.randn((H,), generator=g, device=device) * std
        w[HEAD_KEYS[4]] = torch.randn((V,), generator=g, device=device) * std
        if not tied:
            w[DECODER_KEY] = torch.randn((V, H), generator=g, device=device) * std
        return cls(cfg, w, device, tokenizer, scale)

    @classmethod
    def from_local_dir(cls, path: str, device="cuda:0", max_seq_length: Optional[int] = None,
                       scale: Optional[float] = None) -> "DeviceSparseEncoder":
        """Load a `BertForMaskedLM` checkpoint (e.g. a SPLADE checkpoint) from a local Hugging Face style directory
        (config.json + model.safetensors + vocab.txt).  Nothing is downloaded.  Other architectures raise ValueError."""
        from .tokenizer import NativeWordPieceTokenizer

        cfg, w, lower = load_sparse_checkpoint(path, max_seq_length)
        tok = NativeWordPieceTokenizer.from_vocab_file(os.path.join(path, "vocab.txt"), lower)
        return cls(cfg, w, device, tok, scale)

    # ---------------------------------------------------------------- forward ---------------
    MAX_BATCH_TOKENS = 1 << 16      # tokens of one forward: 256 chunks of 256

    def _token_rows(self, ids2d: np.ndarray, lens: np.ndarray):
        """(token rows [T, hidden] float16 of the packed sequences, un-normalised; cu int32 [B + 1]) on the device: the
        plane mmrag_sparse_pool reads.  The caller holds _launch_lock."""
        ids, pos, cu = self._pack_rows(ids2d, lens)
        d_ids, d_pos, d_cu = self._upload(ids, pos, cu)
        T, B = int(ids.size), len(lens)
        need = _native.sparse_expand_forward_workspace_bytes(self.desc, T, B)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        tok = _native.sparse_expand_forward(self.desc, self._ptrs, d_ids, d_pos, d_cu, int(lens.max()),
                                            self._head_w, self._head_b, self._head_g, self._head_beta,
                                            workspace=self._workspace)
        return tok, d_cu

    def _expand_batch(self, ids2d: np.ndarray, lens: np.ndarray, max_terms: int):
        with self._launch_lock:
            tok, d_cu = self._token_rows(ids2d, lens)
            pooled = _native.sparse_pool(tok, d_cu, self._decoder, self.cfg.hidden, n_rows=int(tok.shape[0]))
            cnt, terms, imps = _native.sparse_select(pooled, self.vocab_bias, self.scale, max_terms, self._skip_bits)
        return cnt.cpu().numpy(), terms.cpu().numpy(), imps.cpu().numpy()

    def expand_ids(self, ids2d: np.ndarray, lens: np.ndarray, max_terms: int):
        """Sparse vectors of token-id rows (row i of `ids2d` [B, W] int32 holds lens[i] ids, truncated to the encoder's
        length): (off int64 [B + 1], terms int32, impacts int32) on the host -- text i's terms[off[i] .. off[i + 1]) in
        ascending term id with impacts 1..255, at most `max_terms` of them, ties at the cut to the lower term id."""
        if not 1 <= int(max_terms) <= _native.MAX_SPARSE_TERMS:
            raise ValueError(f"max_terms must be in 1..{_native.MAX_SPARSE_TERMS}")
        L = min(self.cfg.max_seq_length, self.cfg.max_pos, _native.MAX_SPARSE_CHUNK_TOKENS)
        ids2d = np.asarray(ids2d)
        lens = np.minimum(np.asarray(lens, dtype=np.int32), L)
        if lens.size == 0 or lens.min() <= 0:
            raise ValueError("empty token sequence")
        off = np.zeros(lens.size + 1, np.int64)
        t_parts, i_parts = [], []
        s = 0
        while s < lens.size:
            e, tokens = s, 0
            while e < lens.size and (e == s or tokens + int(lens[e]) <= self.MAX_BATCH_TOKENS):
                tokens += int(lens[e])
                e += 1
            cnt, terms, imps = self._expand_batch(ids2d[s:e], lens[s:e], int(max_terms))
            keep = np.arange(terms.shape[1])[None, :] < cnt[:, None]
            t_parts.append(terms[keep])
            i_parts.append(imps[keep])
            np.cumsum(cnt, out=off[s + 1: e + 1])
            off[s + 1: e + 1] += off[s]
            s = e
        return off, np.concatenate(t_parts).astype(np.int32), np.concatenate(i_parts).astype(np.int32)

    def expand_texts(self, texts: Sequence[str], max_terms: int):
        """expand_ids over the checkpoint's own WordPiece tokenisation ([CLS] ... [SEP])"""
        if self.tokenizer is None:
            raise RuntimeError("this sparse encoder has no tokenizer (load it with from_local_dir or pass one)")
        L = min(self.cfg.max_seq_length, self.cfg.max_pos, _native.MAX_SPARSE_CHUNK_TOKENS)
        texts = [t if t is not None else "" for t in texts]
        if hasattr(self.tokenizer, "encode_batch_arrays"):
            ids, lens = self.tokenizer.encode_batch_arrays(texts, L)
        else:
            rows = [self.tokenizer.encode(t, L) for t in texts]
            lens = np.array([len(r) for r in rows], np.int32)
            ids = np.zeros((len(rows), max(int(lens.max(initial=1)), 1)), np.int32)
            for i, r in enumerate(rows):
                ids[i, : len(r)] = r
        return self.expand_ids(ids, lens, max_terms)

    def token_terms(self, texts: Sequence[str], max_terms: int):
        """The SPLADE-doc query form: a text's own distinct word pieces, each with impact rint(scale) (at most 255), no
        forward pass.  Same return shape as expand_texts; special ids are dropped, the lowest ids kept past max_terms."""
        if self.tokenizer is None:
            raise RuntimeError("this sparse encoder has no tokenizer (load it with from_local_dir or pass one)")
        L = min(self.cfg.max_seq_length, self.cfg.max_pos)
        w = int(min(255, max(1, round(self.scale))))
        off = np.zeros(len(texts) + 1, np.int64)
        parts = []
        for i, t in enumerate(texts):
            ids = np.unique(np.asarray(self.tokenizer.encode(t or "", L), np.int64))
            ids = ids[(ids >= 0) & (ids < self.cfg.vocab)]
            ids = ids[~self._skip_host[ids]][: int(max_terms)]
            parts.append(ids)
            off[i + 1] = off[i] + ids.size
        terms = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
        return off, terms, np.full(terms.size, w, np.int32)

    def terms_to_strings(self, terms: Sequence[int]) -> List[str]:
        """vocabulary strings of term ids (the id itself, as text, without a tokenizer)"""
        if self._id2tok is None and self.tokenizer is not None and getattr(self.tokenizer, "vocab", None):
            tab = [""] * self.cfg.vocab
            for t, i in self.tokenizer.vocab.items():
                if 0 <= i < len(tab):
                    tab[i] = t
            self._id2tok = tab
        if self._id2tok is None:
            return [str(int(t)) for t in terms]
        return [self._id2tok[int(t)] or str(int(t)) for t in terms]


def check_sparse_rows(off, terms, impacts, n_terms: int, m: Optional[int] = None, max_terms: Optional[int] = None,
                      what: str = "sparse"):
    """validated (off int64 [m + 1] from 0, terms int32, impacts int32) of m sparse vectors: terms strictly ascending
    within a vector and inside 0..n_terms, impacts 1..255"""
    off = np.ascontiguousarray(off, np.int64)
    terms = np.ascontiguousarray(terms, np.int32)
    impacts = np.ascontiguousarray(impacts, np.int32)
    if off.ndim != 1 or off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != terms.size:
        raise ValueError(f"{what}: offsets must ascend from 0 to the number of terms")
    if m is not None and off.size != m + 1:
        raise ValueError(f"{what}: {off.size - 1} vectors for {m} rows")
    if terms.shape != impacts.shape or terms.ndim != 1:
        raise ValueError(f"{what}: terms and impacts differ in length")
    if terms.size:
        if terms.min() < 0 or terms.max() >= n_terms:
            raise ValueError(f"{what}: term id outside 0..{n_terms - 1}")
        if impacts.min() < 1 or impacts.max() > 255:
            raise ValueError(f"{what}: impacts must be in 1..255")
        inner = np.ones(terms.size, bool)
        inner[off[:-1][off[:-1] < terms.size]] = False       # the first term of each vector
        if (np.diff(terms) <= 0)[inner[1:]].any():
            raise ValueError(f"{what}: term ids must be distinct and ascending within a vector")
    if max_terms is not None and off.size > 1 and np.diff(off).max() > max_terms:
        raise ValueError(f"{what}: at most {max_terms} terms per vector")
    return off, terms, impacts


class ImpactIndex:
    """The device state of one `VectorIndex`'s learned sparse vectors (its owner holds the lock around every call),
    shaped like `lexical.LexicalIndex`: a forward log of (term, impact) rows, kept on the host too (explanations are
    built from it), and the term-major CSR rebuilt on the device by the first search after a change.  A delete touches
    nothing here: the owner's alive bits filter dead rows."""

    def __init__(self, device, n_terms: int):
        if not 1 <= int(n_terms) <= _native.MAX_SPARSE_VOCAB:
            raise ValueError(f"vocab_size must be in 1..{_native.MAX_SPARSE_VOCAB}")
        self.device = torch.device(device)
        self.n_terms = int(n_terms)
        self.reset()

    def reset(self):
        self.n = 0
        self._off_host = np.zeros(1, np.int64)
        self._term_host = np.zeros(0, np.int32)
        self._imp_host = np.zeros(0, np.int32)
        self._fwd = None                  # (fwd_off, fwd_term, fwd_imp) on the device, of version _fwd_version
        self._version = 0                 # bumped by every change of the forward log
        self._fwd_version = self._csr_version = -1
        self._csr = None
        self._csr_ws = None
        self._search_ws = None
        self.csr_builds = 0               # how many times the CSR was rebuilt (tests, tools)

    @property
    def n_postings(self) -> int:
        return int(self._off_host[-1])

    def append(self, off, terms, impacts):
        """append rows n .. n + m (validated vectors, offsets from 0)"""
        off, terms, impacts = check_sparse_rows(off, terms, impacts, self.n_terms)
        m = off.size - 1
        if m == 0:
            return
        self._off_host = np.concatenate([self._off_host[:-1], self.n_postings + off])
        self._term_host = np.concatenate([self._term_host, terms])
        self._imp_host = np.concatenate([self._imp_host, impacts])
        self.n += m
        self._version += 1

    def append_empty(self, m: int):
        """append m rows without terms (they match nothing)"""
        if m > 0:
            self.append(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))

    def set_rows(self, rows, off, terms, impacts):
        """replace the vectors of `rows` (distinct, inside 0..n)"""
        rows = np.ascontiguousarray(rows, np.int64)
        off, terms, impacts = check_sparse_rows(off, terms, impacts, self.n_terms, rows.size)
        if rows.size == 0:
            return
        if rows.min() < 0 or rows.max() >= self.n or np.unique(rows).size != rows.size:
            raise ValueError("set_sparse: rows must be distinct and inside the collection")
        lens = np.diff(self._off_host)
        lens[rows] = np.diff(off)
        new_off = np.zeros(self.n + 1, np.int64)
        np.cumsum(lens, out=new_off[1:])
        new_term = np.empty(int(new_off[-1]), np.int32)
        new_imp = np.empty(int(new_off[-1]), np.int32)
        keep = np.ones(self.n, bool)
        keep[rows] = False
        old_rows = np.nonzero(keep)[0]
        old_lens = lens[old_rows]
        if old_lens.sum():
            within = np.arange(int(old_lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(old_lens) - old_lens, old_lens)
            src = np.repeat(self._off_host[old_rows], old_lens) + within
            dst = np.repeat(new_off[old_rows], old_lens) + within
            new_term[dst], new_imp[dst] = self._term_host[src], self._imp_host[src]
        set_lens = np.diff(off)
        if set_lens.sum():
            within = np.arange(int(set_lens.sum()), dtype=np.int64) - np.repeat(off[:-1], set_lens)
            dst = np.repeat(new_off[rows], set_lens) + within
            new_term[dst], new_imp[dst] = terms, impacts
        self._off_host, self._term_host, self._imp_host = new_off, new_term, new_imp
        self._version += 1

    def compact(self, keep: np.ndarray):
        """keep only rows `keep` (ascending), renumbered 0 .. len(keep); the CSR is rebuilt by the next search"""
        keep = np.asarray(keep, np.int64)
        off = self._off_host
        lens = off[keep + 1] - off[keep]
        new_off = np.zeros(keep.size + 1, np.int64)
        np.cumsum(lens, out=new_off[1:])
        src = np.repeat(off[keep] - new_off[:-1], lens) + np.arange(int(new_off[-1]), dtype=np.int64)
        self._term_host, self._imp_host = self._term_host[src], self._imp_host[src]
        self._off_host = new_off
        self.n = int(keep.size)
        self._version += 1

    def row_vector(self, row: int) -> Tuple[np.ndarray, np.ndarray]:
        """(terms, impacts) of one stored row, from the host copy of the forward log"""
        lo, hi = int(self._off_host[row]), int(self._off_host[row + 1])
        return self._term_host[lo:hi], self._imp_host[lo:hi]

    def _ensure_csr(self):
        if self._csr is not None and self._csr_version == self._version:
            return self._csr
        dev, n, P, V = self.device, self.n, self.n_postings, self.n_terms
        if self._fwd_version != self._version:
            up = lambda a, dt: _native._pinned_to_device(torch.from_numpy(np.ascontiguousarray(a, dt)), dev)  # noqa: E731
            pad = np.zeros(1, np.int32)
            self._fwd = (up(self._off_host, np.int64), up(np.concatenate([self._term_host, pad]), np.int32),
                         up(np.concatenate([self._imp_host, pad]), np.int32))
            self._fwd_version = self._version
        fwd_off, fwd_term, fwd_imp = self._fwd
        L = _native.lib()
        term_off = torch.empty(V + 1, dtype=torch.int64, device=dev)
        post_row = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        post_imp = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        need = int(L.mmrag_lexical_csr_build_workspace_bytes(n, V))
        if self._csr_ws is None or self._csr_ws.numel() < need:
            self._csr_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _native._check(L.mmrag_lexical_csr_build(fwd_off.data_ptr(), fwd_term.data_ptr(), fwd_imp.data_ptr(), n, P,
                                                     V, term_off.data_ptr(), post_row.data_ptr(), post_imp.data_ptr(),
                                                     self._csr_ws.data_ptr(), self._csr_ws.numel(),
                                                     _native._stream_ptr(dev)), "mmrag_lexical_csr_build")
        self._csr, self._csr_version = (term_off, post_row, post_imp), self._version
        self.csr_builds += 1
        return self._csr

    def topk(self, q_off, q_terms, q_impacts, k: int, alive_bits: Optional[torch.Tensor] = None, cap: int = 0,
             dbg: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scores [B, k] float32 desc, rows [B, k] int64; (-inf, -1) padding) on the device: query i holds the
        distinct terms q_terms[q_off[i] .. q_off[i + 1]) with impacts 1..255, at most 64 of them.  `cap`, `dbg`: the
        test hook of mmrag_impact_topk (candidate capacity; 1 = no bound stages)."""
        if not 1 <= k <= _native.MAX_K_DEEP:
            raise ValueError(f"n_results must be in 1..{_native.MAX_K_DEEP} for sparse search")
        q_off, q_terms, q_impacts = check_sparse_rows(q_off, q_terms, q_impacts, self.n_terms, None,
                                                      _native.MAX_SPARSE_QUERY_TERMS, "sparse query")
        B = q_off.size - 1
        if B < 1:
            raise ValueError("no sparse queries")
        term_off, post_row, post_imp = self._ensure_csr()
        pad = np.zeros(1, np.int32)
        host = np.concatenate([q_off.astype(np.int32), q_terms, pad, q_impacts, pad])
        dev = _native._pinned_to_device(torch.from_numpy(host), self.device)
        nq = q_terms.size + 1
        d_off, d_terms, d_imp = dev[: B + 1], dev[B + 1: B + 1 + nq], dev[B + 1 + nq:]
        need = _native.impact_topk_workspace_bytes(B, self.n, k)
        if self._search_ws is None or self._search_ws.numel() < need:
            self._search_ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        return _native.impact_topk(term_off, post_row, post_imp, self.n_terms, self.n, d_off, d_terms, d_imp, k,
                                   alive_bits, self._search_ws, cap, dbg)
