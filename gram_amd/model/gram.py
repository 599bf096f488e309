"""GRAM model wrapper: the reference's ``src/model/gram.py`` interface over libgram_hip.so.

Same constructor (``GRAM(config)``), same state-dict key layout, same
``load_t5`` / ``load_state_dict`` / ``generate`` signatures as the reference class
(gram.py:14-107,162-165), so ``main_generative_gram.py`` and the runners drive it unchanged.
``generate`` runs entirely on the MI355X through ONE C-ABI call (``gram_generate``): encoder,
late fusion, the beam-shared KV bank, and the Trie-constrained beam search all stay on the
device; there is no PyTorch-op or CPU fallback.

``forward(input_ids, attention_mask, labels=...)`` -- the reference runners' loss call -- and ``score_sequences`` (log p(item | user)
for given candidates) run the teacher-forced decoder pass on the device (``gram_teacher_forced``).  Out of scope (SURVEY.md §8,
training half): the backward pass -- ``loss.backward()`` raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Callable, Dict, Optional

import torch
from torch import nn

from .. import _lib
from ..utils.generation_trie import FlatTrie, Trie


class GenerateOutput(dict):
    """Mapping with attribute access, standing in for HF's BeamSearchEncoderDecoderOutput:
    the runner reads ``prediction["sequences"]`` / ``prediction["sequences_scores"]``
    (single_runner_gram.py:654-655)."""

    __getattr__ = dict.get


class ForwardOutput(dict):
    """What ``GRAM.forward`` returns unless ``return_dict=False``: ``.loss`` (None without labels) and ``.logits`` (B, T, V), like
    HF's Seq2SeqLMOutput; integer indexing walks the non-None fields in that order (``out[0]`` is the loss when there is one)."""

    __getattr__ = dict.get

    def to_tuple(self):
        return tuple(v for v in (self.get("loss"), self.get("logits")) if v is not None)

    def __getitem__(self, k):
        return self.to_tuple()[k] if isinstance(k, (int, slice)) else dict.__getitem__(self, k)


def shift_right(labels: torch.Tensor, start_token: int = 0, pad_token: int = 0) -> torch.Tensor:
    """T5's ``_shift_right`` (gram_t5_modeling.py:935-964): the decoder inputs of teacher forcing -- the start token, then the labels
    without their last position, with the ignored label -100 replaced by the pad token."""
    out = labels.new_zeros(labels.shape)
    out[..., 1:] = labels[..., :-1]
    out[..., 0] = start_token
    return out.masked_fill(out == -100, pad_token)


class _NoBackward(torch.autograd.Function):
    """Carries the teacher-forced loss into autograd so that ``loss.backward()`` fails loudly instead of with torch's "does not
    require grad": the HIP path has no backward yet."""

    @staticmethod
    def forward(ctx, loss, anchor):
        return loss.clone()

    @staticmethod
    def backward(ctx, grad):
        raise NotImplementedError("backward is not implemented on the HIP path")


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted parameter names."""


def _register(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        child = mod._modules.get(p)
        if child is None:
            child = _Node()
            mod.add_module(p, child)
        mod = child
    mod.register_parameter(parts[-1], param)


def relative_position_bucket(rel: torch.Tensor, bidirectional: bool, num_buckets: int, max_distance: int) -> torch.Tensor:
    """Bucket index of a relative position (key - query).  Same integer results as
    T5Attention._relative_position_bucket (gram_t5_modeling.py:398-450), evaluated once on the
    host to build the per-head bias tables the kernels index."""
    rel = rel.to(torch.long)
    out = torch.zeros_like(rel)
    n = num_buckets
    if bidirectional:
        n //= 2
        out += (rel > 0).long() * n
        dist = rel.abs()
    else:
        dist = (-rel).clamp(min=0)
    exact = n // 2
    log_part = exact + (torch.log(dist.float() / exact) / math.log(max_distance / exact) * (n - exact)).long()
    log_part = log_part.clamp(max=n - 1)
    return out + torch.where(dist < exact, dist, log_part)


class GRAM(nn.Module):
    main_input_name = "input_ids"

    def __init__(self, config):
        super().__init__()
        self.config = config
        c = config
        if c.d_kv != 64:
            raise ValueError("gram_amd kernels are built for d_kv == 64 (every T5 checkpoint the reference uses)")
        if getattr(c, "feed_forward_proj", "relu") not in ("relu",):
            raise ValueError("only the ReLU feed-forward of t5-{small,base,large} is on the path")
        self.max_seq_len = getattr(c, "max_seq_len", 128)
        self.max_item_num = getattr(c, "max_item_num", 20)
        self.use_position_embedding = bool(getattr(c, "use_position_embedding", True))
        d, inner, F, V = c.d_model, c.num_heads * c.d_kv, c.d_ff, c.vocab_size
        self.model_dim = d
        dec_layers = c.num_decoder_layers if getattr(c, "num_decoder_layers", None) is not None else c.num_layers
        self._n_enc, self._n_dec = c.num_layers, dec_layers

        def P(*shape):
            return nn.Parameter(torch.empty(*shape, dtype=torch.float32))

        shared = P(V, d)
        _register(self, "shared.weight", shared)
        _register(self, "encoder.encoder.embed_tokens.weight", shared)
        _register(self, "decoder.embed_tokens.weight", shared)

        def attn(prefix, rel):
            _register(self, prefix + ".q.weight", P(inner, d))
            _register(self, prefix + ".k.weight", P(inner, d))
            _register(self, prefix + ".v.weight", P(inner, d))
            _register(self, prefix + ".o.weight", P(d, inner))
            if rel:
                _register(self, prefix + ".relative_attention_bias.weight", P(c.relative_attention_num_buckets, c.num_heads))

        def ff(prefix):
            _register(self, prefix + ".DenseReluDense.wi.weight", P(F, d))
            _register(self, prefix + ".DenseReluDense.wo.weight", P(d, F))

        for i in range(self._n_enc):
            p = f"encoder.encoder.block.{i}.module.layer"
            attn(p + ".0.SelfAttention", i == 0)
            _register(self, p + ".0.layer_norm.weight", P(d))
            ff(p + ".1")
            _register(self, p + ".1.layer_norm.weight", P(d))
        _register(self, "encoder.encoder.final_layer_norm.weight", P(d))
        for i in range(self._n_dec):
            p = f"decoder.block.{i}.layer"
            attn(p + ".0.SelfAttention", i == 0)
            _register(self, p + ".0.layer_norm.weight", P(d))
            attn(p + ".1.EncDecAttention", False)
            _register(self, p + ".1.layer_norm.weight", P(d))
            ff(p + ".2")
            _register(self, p + ".2.layer_norm.weight", P(d))
        _register(self, "decoder.final_layer_norm.weight", P(d))
        if self.use_position_embedding:
            pos = P(self.max_item_num + 1, d)  # one extra for the coarse user prompt (gram.py:23-26)
            _register(self, "position_embedding.weight", pos)
            _register(self, "encoder.position_embedding.weight", pos)
        _register(self, "lm_head.weight", shared if getattr(c, "tie_word_embeddings", True) else P(V, d))
        self._init_weights()
        self._packed = None  # (device, version, handle, keepalive)
        self._version = 0
        self._workspace = None
        self._tail_no_fit = set()  # shapes whose tail-pass workspace did not fit the device (_tail_workspace)
        self._tries: Dict[int, tuple] = {}  # id(trie) -> (trie, FlatTrie)
        # The reference computes in fp32; "f16x3" (two IEEE-half pieces per value, three MFMA products per product) is the cheapest
        # arithmetic that keeps Recall@5 / NDCG@5 within 1e-4 of it, so it is what a drop-in model starts in.
        # GRAM_PRECISION / set_precision() choose another.
        self._precision = os.environ.get("GRAM_PRECISION") or None  # None: the loaded library's default, resolved at first use
        if self._precision is not None and self._precision not in self.PRECISIONS:
            raise ValueError(f"GRAM_PRECISION={self._precision!r}: choose from {self.PRECISIONS}")
        self._pcache = None  # passage cache: dict(x, canon, keys, perm) on the device
        self._stage_caps: Dict[str, int] = {}  # sensitivity sweeps only (set_stage_pieces)

    # ------------------------------------------------------------------ weights
    def _init_weights(self) -> None:
        """Distributions of the reference initialiser (gram_t5_modeling.py:865-929, gram.py:32-33)."""
        c = self.config
        d, dk, H, F = c.d_model, c.d_kv, c.num_heads, c.d_ff
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("layer_norm.weight"):
                    p.fill_(1.0)
                elif name.endswith(".q.weight"):
                    p.normal_(0.0, (d * dk) ** -0.5)
                elif name.endswith((".k.weight", ".v.weight", "wi.weight", "relative_attention_bias.weight")):
                    p.normal_(0.0, d ** -0.5)
                elif name.endswith(".o.weight"):
                    p.normal_(0.0, (H * dk) ** -0.5)
                elif name.endswith("wo.weight"):
                    p.normal_(0.0, F ** -0.5)
                elif name.endswith("position_embedding.weight"):
                    p.normal_(0.0, 0.02)
                else:
                    p.normal_(0.0, 1.0)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._invalidate()
        return out

    def load_t5(self, state_dict):
        """gram.py:162-165: load a plain T5 checkpoint (encoder blocks are not wrapped there:
        ``encoder.block.{i}.layer...``), non-strict, leaving ``position_embedding`` as initialised."""
        remapped = {}
        for k, v in state_dict.items():
            if k.startswith("encoder.block."):
                parts = k.split(".")
                k = "encoder.encoder.block." + parts[2] + ".module." + ".".join(parts[3:])
            elif k.startswith("encoder.") and not k.startswith("encoder.encoder."):
                k = "encoder." + k
            remapped[k] = v
        return self.load_state_dict(remapped, strict=False)

    # "f16" / "bf16": one 16-bit piece per value (11 / 8 significant bits).  "f16x3" / "bf16x3": every value travels as two pieces and
    # every product is three MFMA products (gram_hip.h, gram_split_t): ~2^-22 / ~2^-18 relative error at 3x the MFMA work.
    # The 16-bit type is a property of the library build (gram_piece_format(): libgram_hip.so, the default build, computes on IEEE
    # half; `make PIECE=bf16` builds libgram_hip_bf16.so on bfloat16); the mode's prefix must name the loaded library's type.
    PRECISIONS = ("bf16", "bf16x3", "f16", "f16x3")
    _PIECES = {"bf16": 1, "bf16x3": 2, "f16": 1, "f16x3": 2}

    @staticmethod
    def default_precision() -> str:
        return "f16x3" if _lib.load().gram_piece_format() == 1 else "bf16x3"

    @property
    def precision(self) -> str:
        if self._precision is None:
            self._precision = self.default_precision()
        return self._precision

    def set_precision(self, mode: str) -> None:
        """Arithmetic of the GEMM / attention operands (accumulation, residual stream, softmax and scores are fp32 in
        every mode).  The packed weights depend on it, so changing it re-packs on the next ``generate``."""
        if mode not in self.PRECISIONS:
            raise ValueError(f"unknown precision {mode!r}; choose from {self.PRECISIONS}")
        if mode != self._precision:
            self._precision = mode
            self._invalidate()

    def set_stage_pieces(self, caps: Optional[Dict[str, int]] = None) -> None:
        """Sensitivity sweeps (tests/precision_population.py): stage -> number of pieces its operands keep, for the stages of
        ``_lib.STAGES``; the other stages keep the mode's own count.  The kernels and their cost do not change: the upper pieces of
        a capped stage's weights are zeroed here and those of its activations in generate.hip (gram_debug_set_stage_pieces), which
        is arithmetically the smaller piece count.  The caps are process-wide in the library; ``None`` / ``{}`` lifts them."""
        caps = dict(caps or {})
        for k in caps:
            if k not in _lib.STAGES:
                raise ValueError(f"unknown stage {k!r}; choose from {_lib.STAGES}")
        arr = (C.c_int32 * len(_lib.STAGES))(*[int(caps.get(k, 99)) for k in _lib.STAGES])
        _lib.check(_lib.load().gram_debug_set_stage_pieces(arr if caps else None, len(_lib.STAGES)), "gram_debug_set_stage_pieces")
        if caps != self._stage_caps:
            self._stage_caps = caps
            self._invalidate()

    _max_passage_len = _lib.GRAM_MAX_PASSAGE_LEN  # (class default: a model starts at the short kernel's limit)

    def set_max_passage_len(self, n: int) -> None:
        """Longest (padded) passage the model takes: a multiple of 32 in [128, 512], default 128 (``--item_prompt_max_len`` of the
        reference, arguments.py:293-298).  Above 128 the encoder's self-attention is the tiled kernel for long passages at EVERY
        length (gram_model_set_max_passage_len), so a passage's bits never depend on the batch it was padded with; at 128 the model
        launches what it always launched.  N * L stays within the model's fused limit in every mode (4096 unless raised:
        ``set_max_fused_tokens``).  The passage cache is cleared and its rows become
        ``n`` long.  The kernel indexes the encoder's relative bias by clamp(key - query, -127, 127): a config whose bucket
        function is not constant beyond +-127 (relative_attention_max_distance > 128) is refused for n > 128."""
        n = int(n)
        if n % 32 or not _lib.GRAM_MAX_PASSAGE_LEN <= n <= _lib.GRAM_MAX_LONG_PASSAGE_LEN:
            raise ValueError(f"set_max_passage_len: a multiple of 32 in [{_lib.GRAM_MAX_PASSAGE_LEN}, {_lib.GRAM_MAX_LONG_PASSAGE_LEN}] "
                             f"is supported (got {n})")
        if n > _lib.GRAM_MAX_PASSAGE_LEN:
            c = self.config
            # (the bucket is monotone in the distance: equal at 127 and at n - 1 means constant in between)
            ends = torch.tensor([-(n - 1), -127, 127, n - 1])
            b = relative_position_bucket(ends, True, c.relative_attention_num_buckets, c.relative_attention_max_distance)
            if int(b[0]) != int(b[1]) or int(b[2]) != int(b[3]):
                raise ValueError(f"set_max_passage_len({n}): the relative-position buckets of this config (num_buckets="
                                 f"{c.relative_attention_num_buckets}, max_distance={c.relative_attention_max_distance}) are not constant "
                                 f"beyond distance +-127, which passages longer than {_lib.GRAM_MAX_PASSAGE_LEN} tokens need")
        self._max_passage_len = n
        self._CACHE_L = n
        self._pcache = None  # (rows of another length)
        if self._packed is not None and self._packed[1] == self._version:
            _lib.check(_lib.load().gram_model_set_max_passage_len(self._packed[2], n), "gram_model_set_max_passage_len")

    def _check_passage_len(self, L: int) -> int:
        """The padded passage length of a call, or a ValueError that names the way out."""
        Lp = (int(L) + 31) // 32 * 32
        if Lp > self._max_passage_len:
            hint = (f"call set_max_passage_len({min(Lp, _lib.GRAM_MAX_LONG_PASSAGE_LEN)}) first" if Lp <= _lib.GRAM_MAX_LONG_PASSAGE_LEN
                    else f"set_max_passage_len goes up to {_lib.GRAM_MAX_LONG_PASSAGE_LEN}")
            raise ValueError(f"passages of {L} tokens (padded to {Lp}) exceed this model's limit of {self._max_passage_len}: {hint}")
        return Lp

    _max_fused_tokens = _lib.GRAM_MAX_FUSED_LEN  # (class default: a model starts at the short cross-attention's limit)

    def set_max_fused_tokens(self, n: int) -> None:
        """Longest fused context N * L (passages x padded passage length) the model takes: a multiple of 32 in [4096, 16384],
        default 4096.  The reference's default history (``--max_his 20``: 21 passages) needs 4704 at 224 tokens per passage and
        10752 at 512.  Above 4096 the decoder's cross-attention is the segmented kernel at EVERY length
        (gram_model_set_max_fused_len), so a user's bits never depend on the batch it was padded with; at 4096 the model launches
        what it always launched.  The passage cache stays: cached passages do not depend on N * L.  ``cross_attentions``
        stays limited to 4096 fused tokens; ``passage_attention`` follows the raised limit.  The cross K/V bank is what grows: layers x heads x 64 x (K, V^T) x
        2 B x pieces per fused key and user -- 73.7 KB at T5-base and two pieces, 0.79 GB per user at N * L = 10752; the users per
        call follow from the workspace queries (``max_users_per_call``)."""
        n = int(n)
        if n % 32 or not _lib.GRAM_MAX_FUSED_LEN <= n <= _lib.GRAM_MAX_LONG_FUSED_LEN:
            raise ValueError(f"set_max_fused_tokens: a multiple of 32 in [{_lib.GRAM_MAX_FUSED_LEN}, {_lib.GRAM_MAX_LONG_FUSED_LEN}] "
                             f"is supported (got {n})")
        self._max_fused_tokens = n
        if self._packed is not None and self._packed[1] == self._version:
            _lib.check(_lib.load().gram_model_set_max_fused_len(self._packed[2], n), "gram_model_set_max_fused_len")

    def _check_fused_len(self, N: int, L: int) -> int:
        """The fused length N * (L padded to 32) of a call, or a ValueError that names the way out."""
        S = int(N) * ((int(L) + 31) // 32 * 32)
        if S > self._max_fused_tokens:
            hint = (f"call set_max_fused_tokens({S}) first" if S <= _lib.GRAM_MAX_LONG_FUSED_LEN
                    else f"set_max_fused_tokens goes up to {_lib.GRAM_MAX_LONG_FUSED_LEN}")
            raise ValueError(f"{N} passages of {L} tokens are {S} fused tokens, above this model's limit of {self._max_fused_tokens}: {hint}")
        return S

    def _invalidate(self) -> None:
        self._version += 1
        self._pcache = None  # cached encoder states belong to the old weights

    def _apply(self, fn, *a, **kw):  # .to()/.cuda()/.float() all funnel through here
        out = super()._apply(fn, *a, **kw)
        self._invalidate()
        return out

    def train(self, mode: bool = True):
        # parameters may have been updated by an optimizer while training: repack on leaving train mode
        if self.training != bool(mode):
            self._invalidate()
        return super().train(mode)

    def wrap_encoder(self, use_checkpoint=False):  # API no-ops kept for drop-in compatibility
        pass

    def unwrap_encoder(self):
        pass

    def set_checkpoint(self, use_checkpoint):
        pass

    def forward(self, input_ids=None, attention_mask=None, labels=None, decoder_input_ids=None, decoder_attention_mask=None,
                return_dict=None, output_attentions=None, output_hidden_states=None, **kwargs):
        """GRAM.forward (gram.py:50-60) -> T5ForConditionalGeneration_GRAM.forward (gram_t5.py:181-263) on the device, teacher forced.

        input_ids / attention_mask (B, N, L); labels (B, T) with -100 for ignored positions; decoder_input_ids (B, T) default to
        ``shift_right(labels)``.  ``return_dict=False`` gives ``(loss, logits)`` -- ``(logits,)`` without labels --, anything else a
        ``ForwardOutput`` with ``.loss`` / ``.logits``.  The loss is CrossEntropyLoss(ignore_index=-100): the mean over the labels
        that are not ignored.  ``past_key_values`` and the encoder states are not returned.  There is no backward pass: with grad
        enabled and trainable parameters, ``loss.backward()`` raises NotImplementedError."""
        if self._device().type != "cuda":
            raise NotImplementedError("gram_amd.GRAM.forward runs on a ROCm device (model.to('cuda')); there is no CPU path")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("output_attentions / output_hidden_states are not returned by the HIP path")
        if decoder_attention_mask is not None and not bool(torch.as_tensor(decoder_attention_mask).ne(0).all()):
            raise NotImplementedError("a decoder_attention_mask with masked positions is not supported: the HIP decoder is causal only, "
                                      "as the reference's forward(labels) is")
        for k, v in kwargs.items():
            if v is not None and k not in ("use_cache",):
                raise NotImplementedError(f"forward({k}=...) is not supported by the HIP path")
        if labels is None and decoder_input_ids is None:
            raise ValueError("forward needs labels or decoder_input_ids (as HF's T5ForConditionalGeneration)")
        if input_ids is None or input_ids.dim() != 3:
            raise ValueError("input_ids must be (B, N, L)")
        dev = self._device()
        lab = None if labels is None else self._check_labels(labels.to(dev))
        if lab is not None and lab.dim() != 2:
            raise ValueError("labels must be (B, T)")
        dec = shift_right(lab) if decoder_input_ids is None else decoder_input_ids.to(dev)
        if dec.dim() != 2 or dec.shape[0] != input_ids.shape[0] or (lab is not None and lab.shape != dec.shape):
            raise ValueError("decoder_input_ids / labels must be (B, T) with B = input_ids.shape[0]")
        lab_k = lab if lab is not None else torch.full_like(dec, -100)
        logits, tok, _seq = self._teacher_forced(input_ids, attention_mask, dec[:, None, :], lab_k[:, None, :], want_logits=True)
        logits = logits[:, 0]
        loss = None
        if lab is not None:
            n = int(lab.ne(-100).sum())
            loss = -(tok.double().sum() / n).float() if n else torch.full((), float("nan"), device=dev)
            anchor = self.get_parameter("shared.weight")
            if torch.is_grad_enabled() and anchor.requires_grad:
                loss = _NoBackward.apply(loss, anchor)
        if return_dict is False:
            return (logits,) if loss is None else (loss, logits)
        return ForwardOutput(loss=loss, logits=logits)

    @torch.no_grad()
    def score_sequences(self, input_ids, attention_mask, labels, return_tokens: bool = False, users_per_call: Optional[int] = None):
        """log p(sequence | user) of given candidates, teacher forced: re-ranking a retrieval stage, sampled-negative evaluation,
        checking a beam's ``sequences_scores``.  input_ids / attention_mask (B, N, L); labels (B, C, T) in label form -- no start
        token, -100 after the end.  Returns the (B, C) fp32 sums of the token log-probs (full-vocabulary log_softmax, as a beam's
        running score), and with ``return_tokens`` also the (B, C, T) token log-probs (0 at ignored positions).  Users are scored
        in chunks whose workspace fits the free HBM (``users_per_call`` overrides); a user's scores do not depend on the chunk."""
        if self._device().type != "cuda":
            raise NotImplementedError("gram_amd.GRAM.score_sequences runs on a ROCm device (model.to('cuda')); there is no CPU path")
        if input_ids.dim() != 3 or labels.dim() != 3 or labels.shape[0] != input_ids.shape[0]:
            raise ValueError("input_ids must be (B, N, L) and labels (B, C, T)")
        lab = self._check_labels(labels.to(self._device()))
        _logits, tok, seq = self._teacher_forced(input_ids, attention_mask, shift_right(lab), lab, want_logits=False,
                                                 users_per_call=users_per_call)
        return (seq, tok) if return_tokens else seq

    @torch.no_grad()
    def score_all_items(self, input_ids, attention_mask, prefix_allowed_tokens_fn, candidates, length_penalty: Optional[float] = None,
                        users_per_call: Optional[int] = None):
        """log p(item | user) of EVERY candidate in one decoder pass: the exact rank of a held-out item, full-ranking metrics at any
        cut-off (``gram_amd.utils.evaluate.full_ranking``), an exact check on what beam search missed.  input_ids / attention_mask
        (B, N, L); ``prefix_allowed_tokens_fn`` the Trie closure ``generate`` takes; ``candidates`` the token sequences the Trie was
        built from (the list ``sequence_items`` takes).  Returns (B, len(candidates)) fp32: column i is the value ``score_sequences``
        returns for ``candidates[i]`` -- the decoder runs on one row per internal Trie node instead of one per (candidate, position),
        and computes the same expressions.  Two candidates that spell one sequence get one score, in
        two columns: give ``full_ranking`` the identities ``sequence_ids=FlatTrie(trie).item_ranks(candidates)`` so that such a
        sequence is ranked once.  With ``length_penalty`` the sums are divided by ``len ** length_penalty`` (len = the label count, EOS included; the power in
        float64), as BeamHypotheses.add does: the columns are then comparable with ``sequences_scores``.  Users are scored in
        chunks whose workspace fits the free HBM (``users_per_call`` overrides); a user's scores do not depend on the chunk."""
        if self._device().type != "cuda":
            raise NotImplementedError("gram_amd.GRAM.score_all_items runs on a ROCm device (model.to('cuda')); there is no CPU path")
        if input_ids.dim() != 3:
            raise ValueError("input_ids must be (B, N, L)")
        if prefix_allowed_tokens_fn is None or self._closure_trie(prefix_allowed_tokens_fn) is None:
            raise ValueError("score_all_items needs the Trie closure form of prefix_allowed_tokens_fn (the Trie is what is scored)")
        if len(candidates) < 1:
            raise ValueError("score_all_items: `candidates` is empty")
        dev = self._device()
        V = int(self.config.vocab_size)
        flat = self._flat_trie(prefix_allowed_tokens_fn)
        rows, tables = flat.decoder_rows_on(dev, start_token=int(self.config.decoder_start_token_id))
        _ranks_host, ranks = flat.item_ranks_on(dev, candidates)
        _ctrie, (t_off, t_tok, t_node) = flat.to_device(dev)
        outs, _Lp = self._tf_chunks(input_ids, attention_mask, None, None,
                                    lambda cid, cmask, handle, ws, _dec, _lab, *comp: torch.ops.gram.score_trie(
                                        cid, cmask, handle, ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len),
                                        *tables, int(rows.n_leaves), V, False, *comp)[0],
                                    users_per_call=users_per_call, trie_rows=(int(rows.Q), int(rows.n_leaves)))
        leaf = outs[0] if len(outs) == 1 else torch.cat(outs)
        scores = leaf.index_select(1, ranks.to(torch.int64))
        if length_penalty is not None:
            lens = torch.tensor([len(c) - 1 for c in candidates], dtype=torch.float64, device=dev)  # labels: the start token is not one
            scores = (scores.double() / lens ** float(length_penalty)).float()
        return scores

    def _check_labels(self, labels: torch.Tensor) -> torch.Tensor:
        V = self.config.vocab_size
        if labels.numel() and not bool(((labels >= 0) & (labels < V) | (labels == -100)).all()):
            raise ValueError(f"labels must lie in [0, {V}) or be -100 (ignored)")
        return labels

    def max_users_per_call_tf(self, N: int, L: int, C_: int, T: int, want_logits: bool = False, limit: int = 1 << 20,
                              headroom: float = 0.9, extra_per_user: int = 0) -> int:
        """Largest B <= limit whose teacher-forced workspace (gram_workspace_bytes_tf) and outputs fit the free HBM, net of what a
        reserved passage cache will still allocate (``reserve_passage_cache``).  ``extra_per_user``: further output bytes per user
        (the attention buffers of ``cross_attentions`` / ``passage_attention``)."""
        self._check_fused_len(N, L)
        handle = self._pack()
        lib = _lib.load()
        Lp = (int(L) + 31) // 32 * 32
        per_user_out = C_ * T * 4 * (2 + (self.config.vocab_size if want_logits else 0)) + int(extra_per_user)

        def need(b):
            w = lib.gram_workspace_bytes_tf(handle, b, N, Lp, C_, T)
            return -1 if w < 0 else w + b * per_user_out

        return self._largest_chunk(need, limit, headroom)

    def max_users_per_call_trie(self, N: int, L: int, Q: int, n_out: int, limit: int = 1 << 20, headroom: float = 0.9) -> int:
        """``max_users_per_call_tf`` for the one-pass scoring of a Trie (gram_workspace_bytes_trie): Q decoder rows and ``n_out``
        fp32 outputs per user."""
        self._check_fused_len(N, L)
        handle = self._pack()
        lib = _lib.load()
        Lp = (int(L) + 31) // 32 * 32

        def need(b):
            w = lib.gram_workspace_bytes_trie(handle, b, N, Lp, Q)
            return -1 if w < 0 else w + b * 4 * int(n_out)

        return self._largest_chunk(need, limit, headroom)

    def _largest_chunk(self, need, limit: int, headroom: float) -> int:
        """Largest B <= limit with 0 <= need(B) <= the free HBM (this model's workspace counts as free) * headroom, net of what a
        reserved passage cache will still allocate; at least 1."""
        dev = self._device()
        free, _total = torch.cuda.mem_get_info(dev)
        if self._workspace is not None and self._workspace.device == dev:
            free += self._workspace.numel()
        pc_have = 0 if self._pcache is None else int(self._pcache["x"].shape[0])
        pc_more = max(0, int(getattr(self, "_pcache_reserve", 0)) - pc_have)
        budget = int(free * headroom) - pc_more * self._CACHE_L * (self.config.d_model * 4 + 4)
        lo, hi = 1, max(1, int(limit))
        if 0 <= need(hi) <= budget:
            return hi
        while lo < hi:  # bytes grow monotonically with B
            mid = (lo + hi + 1) // 2
            if 0 <= need(mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def _tf_chunks(self, input_ids, attention_mask, dec, lab, call, want_logits: bool = False, extra_bytes=None,
                   users_per_call: Optional[int] = None, trie_rows=None):
        """The teacher-forced pass over user chunks whose workspace and outputs fit the free HBM: ``call(ids, mask, handle, workspace,
        dec, lab, compaction fields)`` per chunk -> (the list of its results, the padded passage length).  ``extra_bytes(Lp)``: further
        output bytes per user.  ``trie_rows=(Q, n_out)``: the one-pass scoring of a Trie instead -- Q decoder rows and n_out fp32
        outputs per user, the workspace of gram_workspace_bytes_trie, no dec / lab (``call`` gets None for both)."""
        self._check_passage_len(input_ids.shape[-1])
        self._check_fused_len(input_ids.shape[1], input_ids.shape[2])
        handle = self._pack()
        lib = _lib.load()
        dev = self._device()
        B, N, L = input_ids.shape
        ids = input_ids.to(dev, torch.int64)
        mask = attention_mask.to(dev).ne(0).view(torch.uint8) if attention_mask.dtype != torch.bool else attention_mask.to(dev).view(torch.uint8)
        Lp = (L + 31) // 32 * 32  # masked padding is invisible to attention: pad L to the kernel tile (as generate)
        if Lp != L:
            ids = torch.nn.functional.pad(ids, (0, Lp - L))
            mask = torch.nn.functional.pad(mask, (0, Lp - L))
        if trie_rows is None:
            _, Cn, T = dec.shape
            if not 1 <= T <= _lib.GRAM_MAX_DEC_LEN:
                raise ValueError(f"sequences of 1..{_lib.GRAM_MAX_DEC_LEN} positions are supported (got {T})")
            dec = dec.to(dev, torch.int32).contiguous()
            lab = lab.to(dev, torch.int32).contiguous()
            step = int(users_per_call) if users_per_call else self.max_users_per_call_tf(
                N, Lp, Cn, T, want_logits, limit=B, extra_per_user=extra_bytes(Lp) if extra_bytes else 0)
            ws_bytes = lambda nb: lib.gram_workspace_bytes_tf(handle, nb, N, Lp, Cn, T)  # noqa: E731
            size = f"C={Cn} T={T}"
        else:
            Qr, n_out = trie_rows
            step = int(users_per_call) if users_per_call else self.max_users_per_call_trie(N, Lp, Qr, n_out, limit=B)
            ws_bytes = lambda nb: lib.gram_workspace_bytes_trie(handle, nb, N, Lp, Qr)  # noqa: E731
            size = f"Q={Qr}"
        from .. import ops as _ops  # noqa: F401  (registers torch.ops.gram.*)
        outs = []
        for b0 in range(0, B, max(1, step)):
            b1 = min(B, b0 + max(1, step))
            nb = b1 - b0
            cid, cmask = ids[b0:b1].contiguous(), mask[b0:b1].contiguous()
            comp, _harvest = self._plan(cid, cmask, nb, N, Lp)
            need = ws_bytes(nb)
            if need < 0:
                raise _lib.GramHipError(f"unsupported problem size B={nb} N={N} L={Lp} {size} (N <= max_item_num+1, L <= {self._max_passage_len}, "
                                        f"N*L <= {self._max_fused_tokens}, T <= {_lib.GRAM_MAX_DEC_LEN})")
            ws = self._ensure_workspace(need)
            if trie_rows is not None:
                cdec = clab = None
            else:
                # (a chunk's slice of dec / lab starts wherever the rows before it end: a copy is 16-byte aligned, as the ops require)
                cdec, clab = (dec[b0:b1], lab[b0:b1]) if dec[b0:b1].data_ptr() % 16 == 0 else (dec[b0:b1].clone(), lab[b0:b1].clone())
            outs.append(call(cid, cmask, int(handle), ws, cdec, clab, *self._comp_args(comp)))
        return outs, Lp

    def _teacher_forced(self, input_ids, attention_mask, dec, lab, want_logits: bool, users_per_call: Optional[int] = None):
        """(logits (B,C,T,V) or empty, token log-probs (B,C,T), sequence sums (B,C)) over user chunks of torch.ops.gram.teacher_forced."""
        V = int(self.config.vocab_size)
        outs, _Lp = self._tf_chunks(input_ids, attention_mask, dec, lab,
                                    lambda cid, cmask, handle, ws, cdec, clab, *comp: torch.ops.gram.teacher_forced(
                                        cid, cmask, handle, ws, cdec, clab, V, bool(want_logits), *comp),
                                    want_logits=want_logits, users_per_call=users_per_call)
        if len(outs) == 1:
            return outs[0]
        return tuple(torch.cat([o[i] for o in outs]) if (i or want_logits) else outs[0][0] for i in range(3))

    # ------------------------------------------------------------------ cross-attention probabilities, per-passage scores
    def _teacher_forced_attn(self, input_ids, attention_mask, dec, lab, want_probs: bool, want_scores: bool,
                             users_per_call: Optional[int] = None):
        """(probs (nl,B,H,C*T,N*Lp) or None, token_scores (B,C*T,N*Lp) or None, passage_scores (B,C*T,N) or None, Lp) over user chunks
        of torch.ops.gram.teacher_forced_attn, with the attention buffers counted in the chunk budget."""
        if attention_mask.shape != input_ids.shape:
            raise ValueError("attention_mask must have input_ids' shape (B, N, L)")
        S = int(input_ids.shape[1]) * ((int(input_ids.shape[2]) + 31) // 32 * 32)
        if S > _lib.GRAM_MAX_FUSED_LEN:
            raise ValueError(f"cross-attention probabilities are limited to {_lib.GRAM_MAX_FUSED_LEN} fused tokens (got N*L = {S}): "
                             f"cross_attentions and passage_attention(fused=False) do not take the longer contexts "
                             f"set_max_fused_tokens allows (passage_attention's default path does)")
        V, H, nl = int(self.config.vocab_size), int(self.config.num_heads), int(self.config.num_decoder_layers)
        N, Q = input_ids.shape[1], dec.shape[1] * dec.shape[2]

        def attn_bytes(Lp):  # per user: every layer's probabilities or one layer of scratch, the token and passage scores
            return 4 * Q * ((nl if want_probs else 1) * H * N * Lp + ((N * Lp + N) if want_scores else 0))

        outs, Lp = self._tf_chunks(input_ids, attention_mask, dec, lab,
                                   lambda cid, cmask, handle, ws, cdec, clab, *comp: torch.ops.gram.teacher_forced_attn(
                                       cid, cmask, handle, ws, cdec, clab, V, nl, H, bool(want_probs), bool(want_scores), *comp),
                                   extra_bytes=attn_bytes, users_per_call=users_per_call)
        probs = (outs[0][0] if len(outs) == 1 else torch.cat([o[0] for o in outs], 1)) if want_probs else None
        tsc, psc = ((outs[0][i] if len(outs) == 1 else torch.cat([o[i] for o in outs])) if want_scores else None for i in (1, 2))
        return probs, tsc, psc, Lp

    @torch.no_grad()
    def cross_attentions(self, input_ids, attention_mask, labels=None, decoder_input_ids=None, users_per_call: Optional[int] = None):
        """HF's ``cross_attentions`` of the teacher-forced pass: a tuple of ``num_decoder_layers`` fp32 tensors (B, H, T, N*L), the
        softmax weights of every decoder position over the user's fused keys (masked keys exactly 0; a user without a valid key:
        uniform).  labels (B, T) in label form (decoder inputs = ``shift_right(labels)``) or decoder_input_ids (B, T) as given;
        ``decoder_input_ids = zeros(B, 1)`` is the first generated token's cross-attention -- every beam's at step 0 -- which
        ``get_crossattention_scores`` consumes.  Computed on the device by a kernel of its own next to the pass's cross-attention
        (the same operands and product order); a user's result does not depend on the chunk (``users_per_call``)."""
        if self._device().type != "cuda":
            raise NotImplementedError("gram_amd.GRAM.cross_attentions runs on a ROCm device (model.to('cuda')); there is no CPU path")
        if labels is None and decoder_input_ids is None:
            raise ValueError("cross_attentions needs labels or decoder_input_ids")
        if input_ids is None or input_ids.dim() != 3:
            raise ValueError("input_ids must be (B, N, L)")
        dev = self._device()
        lab = None if labels is None else self._check_labels(labels.to(dev))
        dec = shift_right(lab) if decoder_input_ids is None else decoder_input_ids.to(dev)
        if dec.dim() != 2 or dec.shape[0] != input_ids.shape[0] or (lab is not None and lab.shape != dec.shape):
            raise ValueError("decoder_input_ids / labels must be (B, T) with B = input_ids.shape[0]")
        lab_k = lab if lab is not None else torch.full_like(dec, -100)
        probs, _t, _p, Lp = self._teacher_forced_attn(input_ids, attention_mask, dec[:, None, :], lab_k[:, None, :], True, False, users_per_call)
        nl, B, H, T, _ = probs.shape
        N, L = input_ids.shape[1:]
        probs = probs.view(nl, B, H, T, N, Lp)[..., :L].reshape(nl, B, H, T, N * L)  # (a view when L % 32 == 0)
        return tuple(probs[i] for i in range(nl))

    @torch.no_grad()
    def _teacher_forced_scores(self, input_ids, attention_mask, dec, lab, users_per_call: Optional[int] = None):
        """(token_scores (B,C*T,N*Lp), passage_scores (B,C*T,N), Lp) over user chunks of torch.ops.gram.teacher_forced_scores: the
        heads are summed inside the kernel, so the chunk budget counts the two results only -- no term in H."""
        if attention_mask.shape != input_ids.shape:
            raise ValueError("attention_mask must have input_ids' shape (B, N, L)")
        if self._max_fused_tokens <= _lib.GRAM_MAX_FUSED_LEN:
            raise ValueError("passage_attention(fused=True) runs on a model whose fused limit was raised: call set_max_fused_tokens(n) "
                             f"with n > {_lib.GRAM_MAX_FUSED_LEN} first")
        V = int(self.config.vocab_size)
        N, Q = input_ids.shape[1], dec.shape[1] * dec.shape[2]
        outs, Lp = self._tf_chunks(input_ids, attention_mask, dec, lab,
                                   lambda cid, cmask, handle, ws, cdec, clab, *comp: torch.ops.gram.teacher_forced_scores(
                                       cid, cmask, handle, ws, cdec, clab, V, *comp),
                                   extra_bytes=lambda Lp: 4 * Q * (N * Lp + N), users_per_call=users_per_call)
        tsc, psc = (outs[0][i] if len(outs) == 1 else torch.cat([o[i] for o in outs]) for i in (0, 1))
        return tsc, psc, Lp

    @torch.no_grad()
    def passage_attention(self, input_ids, attention_mask, labels, users_per_call: Optional[int] = None,
                          fused: Optional[bool] = None):
        """Which passages the decoder read, at every position of given sequences: labels (B, C, T) as for ``score_sequences`` (a
        generated sequence as labels gives the attribution of that hypothesis).  Returns ``(token_scores (B, C, T, N, L),
        passage_scores (B, C, T, N))``: the cross-attention weights summed over decoder layers and heads, and per passage their sum
        over its valid keys / (valid keys * layers * heads) -- ``get_crossattention_scores``'s two results at every position; NaN for a
        passage without a valid key.  A user's result does not depend on the chunk.

        ``fused``: ``False`` reduces one layer of per-head probabilities (B, H, C*T, N*L) at a time on the device and stops at 4096
        fused tokens; ``True`` sums the heads inside the kernel (gram_teacher_forced_scores) -- no per-head buffer, up to 16 384 fused
        tokens, on a model raised by ``set_max_fused_tokens``.  ``None`` (default): ``False`` up to 4096 fused tokens, ``True``
        above.  The two agree within the rounding of the summation order, not bit for bit."""
        if input_ids.dim() == 3:  # which path, and its refusals, before anything touches a device
            S = input_ids.shape[1] * ((input_ids.shape[2] + 31) // 32 * 32)
            if fused is None:
                fused = S > _lib.GRAM_MAX_FUSED_LEN
                if fused:
                    self._check_fused_len(input_ids.shape[1], input_ids.shape[2])  # (a default model: names set_max_fused_tokens)
            elif fused and self._max_fused_tokens <= _lib.GRAM_MAX_FUSED_LEN:
                raise ValueError("passage_attention(fused=True) runs on a model whose fused limit was raised: call "
                                 f"set_max_fused_tokens(n) with n > {_lib.GRAM_MAX_FUSED_LEN} first")
            elif not fused and S > _lib.GRAM_MAX_FUSED_LEN:
                raise ValueError(f"cross-attention probabilities are limited to {_lib.GRAM_MAX_FUSED_LEN} fused tokens (got N*L = {S}): "
                                 f"passage_attention(fused=False) holds one layer of them; fused=None or True takes the longer contexts")
        if self._device().type != "cuda":
            raise NotImplementedError("gram_amd.GRAM.passage_attention runs on a ROCm device (model.to('cuda')); there is no CPU path")
        if input_ids.dim() != 3 or labels.dim() != 3 or labels.shape[0] != input_ids.shape[0]:
            raise ValueError("input_ids must be (B, N, L) and labels (B, C, T)")
        lab = self._check_labels(labels.to(self._device()))
        B, N, L = input_ids.shape
        if fused:
            tsc, psc, Lp = self._teacher_forced_scores(input_ids, attention_mask, shift_right(lab), lab, users_per_call)
        else:
            _pr, tsc, psc, Lp = self._teacher_forced_attn(input_ids, attention_mask, shift_right(lab), lab, False, True, users_per_call)
        _, Cn, T = lab.shape
        return tsc.view(B, Cn, T, N, Lp)[..., :L], psc.view(B, Cn, T, N)

    @staticmethod
    def get_crossattention_scores(cross_attentions, attention_mask, b_idx: int = 0):
        """The reference's ``GRAM.get_crossattention_scores`` (src/model/gram.py:109-138): how much the FIRST generated token attends
        to every key and to every passage of user ``b_idx``.  cross_attentions: ``[token][layer]`` of (B, H, 1, N*L) tensors --
        ``[model.cross_attentions(ids, mask, decoder_input_ids=zeros(B, 1))]`` --, attention_mask (1, N, L): that user's.  Returns
        ``(token_scores, scores)``: the weights summed over layers and heads as a nested list [N][L] (masked keys 0), and a (1, N)
        tensor of per-passage means, sum over the passage's valid keys / (valid keys * layers * heads) (NaN for a passage without
        one).  Plain torch: works on CPU tensors."""
        valid = torch.as_tensor(attention_mask).ne(0)
        if valid.dim() != 3 or valid.shape[0] != 1:
            raise ValueError("attention_mask must be (1, N, L): the mask of user b_idx")
        w = torch.stack([layer[b_idx] for layer in cross_attentions[0]])  # (layers, H, 1, N*L): the first token
        if w.dim() != 4 or w.shape[2] != 1:
            raise ValueError("cross_attentions must hold (B, H, 1, N*L) tensors: one decoder position")
        n_layers, H = w.shape[:2]
        _, N, L = valid.shape
        w = w.reshape(1, n_layers, H, N, L).masked_fill(~valid.to(w.device)[:, None, None], 0.0)
        per_key = w.sum(dim=(1, 2))  # (1, N, L)
        scores = w.sum(dim=(1, 2, 4)) / (valid.to(w.device).sum(dim=2) * (n_layers * H))
        return per_key[0].tolist(), scores

    # ------------------------------------------------------------------ device packing
    def _device(self) -> torch.device:
        return self.get_parameter("shared.weight").device

    def _pack(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(
                "gram_amd.GRAM.generate needs the model on a ROCm device (model.to('cuda')); there is no CPU path"
            )
        if self._packed is not None and self._packed[0] == dev and self._packed[1] == self._version:
            return self._packed[2]
        lib = _lib.load()
        if self._packed is not None:
            lib.gram_model_destroy(self._packed[2])
            self._packed = None
        c = self.config
        H = c.num_heads
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        keep = []

        def f32(t):
            t = t.to(dev, torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        pieces = self._PIECES[self.precision]
        f16 = lib.gram_piece_format() == 1
        if self.precision.startswith("f16") != f16:
            raise _lib.GramHipError(f"precision {self.precision!r} needs the {'f16' if not f16 else 'bf16'} build of libgram_hip "
                                    f"(loaded: {_lib.LIB_PATH}; GRAM_LIB selects another build)")
        tdt = torch.float16 if f16 else torch.bfloat16
        w_scales = []

        caps = self._stage_caps

        def b16(t, stage=None, row_caps=None, no_scale=False):
            """[out][in] fp32 -> the MFMA weight operand: one 16-bit matrix, or (two-piece mode) the INTERLEAVED [out][in/32][2][32]
            matrix of W = p0 + p1, p0 = r16(W), p1 = r16(W - p0): a 64-column k-tile holds both pieces of a 32-column block.
            stage / row_caps: sensitivity sweeps (set_stage_pieces) -- the upper piece is zeroed (per row: row_caps)."""
            t = t.to(dev, torch.float32)
            # f16 build: the matrix is scaled by a power of two so that its largest entry sits in [2^13, 2^14) -- the low pieces of
            # small weights then stay normal numbers (an f16 subnormal keeps fewer bits); the GEMM multiplies its result by the
            # inverse (gram_model_desc_t.w_scales).  The 16-bit lm_head of the one-piece mode is read unscaled by the beam kernel.
            scale = 1.0
            if f16 and not (no_scale and pieces == 1):
                amax = float(t.abs().max())
                if amax > 0.0 and math.isfinite(amax):
                    scale = 2.0 ** (13 - math.floor(math.log2(amax)))
                t = t * scale
            w_scales.append(scale)
            if pieces == 1:
                t = t.to(tdt).contiguous()
            else:
                ps, r = [], t.clone()
                for _ in range(pieces):
                    ps.append(r.to(tdt))
                    r -= ps[-1].float()
                cap = caps.get(stage, 99) if stage else 99
                for j in range(pieces):
                    if j >= cap:
                        ps[j].zero_()
                    elif row_caps is not None:
                        ps[j][row_caps.to(dev) <= j] = 0
                t = _lib.interleave(torch.stack(ps))
            keep.append(t)
            return t.data_ptr()

        def ptr_array(vals):
            arr = (C.c_void_p * len(vals))(*vals)
            keep.append(arr)
            return C.cast(arr, C.POINTER(C.c_void_p))

        # T5LayerNorm folding (gram_norm_fusion_t): the gain g of the norm in front of a Linear is folded into
        # that Linear's columns (W[n][k] * g[k], in fp32, then one bf16 rounding); the 1/rms factor is applied
        # per row in the GEMM epilogue.  GRAM_FOLD_NORM=0 keeps the separate norm kernels (A/B, debugging).
        fold = os.environ.get("GRAM_FOLD_NORM", "1") != "0" or pieces > 1

        def lin(wname, gname, stage):
            w = sd[wname].to(dev, torch.float32)
            return b16(w * sd[gname].to(dev, torch.float32)[None, :], stage) if fold else b16(w, stage)

        def qkv(prefix, gname, stage):
            w = torch.cat([sd[prefix + ".q.weight"], sd[prefix + ".k.weight"], sd[prefix + ".v.weight"]], 0).to(dev, torch.float32)
            return b16(w * sd[gname].to(dev, torch.float32)[None, :], stage) if fold else b16(w, stage)

        # relative-bias tables: encoder [H][255] by (key - query + 127), decoder [H][GRAM_MAX_DEC_LEN] by distance
        nb, md = c.relative_attention_num_buckets, c.relative_attention_max_distance
        rel = torch.arange(-127, 128)
        enc_tab = sd["encoder.encoder.block.0.module.layer.0.SelfAttention.relative_attention_bias.weight"].cpu().float()
        enc_bias = enc_tab[relative_position_bucket(rel, True, nb, md)].t().contiguous()  # (H,255)
        dist = torch.arange(0, _lib.GRAM_MAX_DEC_LEN)
        dec_tab = sd["decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].cpu().float()
        dec_bias = dec_tab[relative_position_bucket(-dist, False, nb, md)].t().contiguous()  # (H, GRAM_MAX_DEC_LEN)

        e = "encoder.encoder.block.{}.module.layer"
        dd = "decoder.block.{}.layer"
        ne, nd = self._n_enc, self._n_dec
        wkv_all = torch.cat(
            [torch.cat([sd[dd.format(i) + ".1.EncDecAttention.k.weight"], sd[dd.format(i) + ".1.EncDecAttention.v.weight"]], 0)
             for i in range(nd)], 0)
        inner_ = H * c.d_kv  # rows of wkv_all: per layer the K rows, then the V rows
        kv_row_caps = None
        if "bank_k" in caps or "bank_v" in caps:
            kv_row_caps = torch.tensor([caps.get("bank_k", 99), caps.get("bank_v", 99)]).repeat_interleave(inner_).repeat(nd)
        desc = _lib.ModelDesc(
            vocab=c.vocab_size, d_model=c.d_model, d_ff=c.d_ff, n_heads=H, n_enc_layers=ne, n_dec_layers=nd,
            max_passages=self.max_item_num + 1, tie_word_embeddings=int(bool(getattr(c, "tie_word_embeddings", True))),
            use_position_embedding=int(self.use_position_embedding), fold_norm=int(fold), eps=float(c.layer_norm_epsilon),
            embed_f32=f32(sd["shared.weight"]), lm_head_bf16=b16(sd["lm_head.weight"], "lm_head", no_scale=True),
            pos_emb_f32=f32(sd["position_embedding.weight"]) if self.use_position_embedding else None,
            enc_bias_f32=f32(enc_bias), dec_bias_f32=f32(dec_bias),
            enc_final_ln=f32(sd["encoder.encoder.final_layer_norm.weight"]),
            dec_final_ln=f32(sd["decoder.final_layer_norm.weight"]),
            enc_ln1=ptr_array([f32(sd[e.format(i) + ".0.layer_norm.weight"]) for i in range(ne)]),
            enc_wqkv=ptr_array([qkv(e.format(i) + ".0.SelfAttention", e.format(i) + ".0.layer_norm.weight", "enc_attn") for i in range(ne)]),
            enc_wo=ptr_array([b16(sd[e.format(i) + ".0.SelfAttention.o.weight"], "enc_attn") for i in range(ne)]),
            enc_ln2=ptr_array([f32(sd[e.format(i) + ".1.layer_norm.weight"]) for i in range(ne)]),
            enc_wi=ptr_array([lin(e.format(i) + ".1.DenseReluDense.wi.weight", e.format(i) + ".1.layer_norm.weight", "enc_ffn") for i in range(ne)]),
            enc_wo2=ptr_array([b16(sd[e.format(i) + ".1.DenseReluDense.wo.weight"], "enc_ffn") for i in range(ne)]),
            dec_ln1=ptr_array([f32(sd[dd.format(i) + ".0.layer_norm.weight"]) for i in range(nd)]),
            dec_wqkv=ptr_array([qkv(dd.format(i) + ".0.SelfAttention", dd.format(i) + ".0.layer_norm.weight", "dec_self") for i in range(nd)]),
            dec_wo=ptr_array([b16(sd[dd.format(i) + ".0.SelfAttention.o.weight"], "dec_self") for i in range(nd)]),
            dec_ln2=ptr_array([f32(sd[dd.format(i) + ".1.layer_norm.weight"]) for i in range(nd)]),
            dec_wq_x=ptr_array([lin(dd.format(i) + ".1.EncDecAttention.q.weight", dd.format(i) + ".1.layer_norm.weight", "dec_cross") for i in range(nd)]),
            dec_wo_x=ptr_array([b16(sd[dd.format(i) + ".1.EncDecAttention.o.weight"], "dec_cross") for i in range(nd)]),
            dec_ln3=ptr_array([f32(sd[dd.format(i) + ".2.layer_norm.weight"]) for i in range(nd)]),
            dec_wi=ptr_array([lin(dd.format(i) + ".2.DenseReluDense.wi.weight", dd.format(i) + ".2.layer_norm.weight", "dec_ffn") for i in range(nd)]),
            dec_wo2=ptr_array([b16(sd[dd.format(i) + ".2.DenseReluDense.wo.weight"], "dec_ffn") for i in range(nd)]),
            dec_wkv_x_all=b16(wkv_all, None, kv_row_caps),
            pieces=pieces, lm_head_f32=f32(sd["lm_head.weight"]) if pieces > 1 else None,
        )
        # b16() ran in the field order of the constructor call above: lm_head first, then the per-layer families, then wkv_all.
        # gram_model_desc_t.w_scales wants [enc_wqkv][enc_wo][enc_wi][enc_wo2][dec_wqkv][dec_wo][dec_wq_x][dec_wo_x][dec_wi][dec_wo2][wkv][lm_head]
        assert len(w_scales) == 4 * ne + 6 * nd + 2
        order = w_scales[1:] + w_scales[:1]
        arr = (C.c_float * len(order))(*order)
        keep.append(arr)
        desc.w_scales = C.cast(arr, C.POINTER(C.c_float))
        handle = lib.gram_model_create(C.byref(desc))
        if not handle:
            raise _lib.GramHipError("gram_model_create rejected the configuration (dims must be multiples of 128, heads <= 16)")
        self._packed = (dev, self._version, handle, keep)
        if self._max_passage_len != _lib.GRAM_MAX_PASSAGE_LEN:
            _lib.check(lib.gram_model_set_max_passage_len(handle, self._max_passage_len), "gram_model_set_max_passage_len")
        if self._max_fused_tokens != _lib.GRAM_MAX_FUSED_LEN:
            _lib.check(lib.gram_model_set_max_fused_len(handle, self._max_fused_tokens), "gram_model_set_max_fused_len")
        self._build_token_tables(handle, keep)
        return handle

    def _build_token_tables(self, handle, keep) -> None:
        """Layer 0's q|k|v per token (gram_hip.h, gram_model_build_token_tables): computed once per handle, on the device, by the
        path's own kernels; the tables live as long as the handle, the build's scratch goes back to the allocator at once.
        GRAM_TOKEN_TABLES=0 (or unfolded norms) leaves the handle without tables: layer 0 then runs its QKV GEMMs."""
        lib = _lib.load()
        self._token_tables = None  # (the uint8 tensor behind both tables: kept by name for the tests)
        need = lib.gram_token_tables_bytes(handle)
        if need <= 0 or os.environ.get("GRAM_TOKEN_TABLES", "1") == "0":
            return
        dev = self._device()
        tables = torch.empty(int(need), dtype=torch.uint8, device=dev)
        scratch = torch.empty(int(lib.gram_token_tables_workspace_bytes(handle)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gram_model_build_token_tables(handle, tables.data_ptr(), tables.numel(), scratch.data_ptr(), scratch.numel(),
                                                         torch.cuda.current_stream(dev).cuda_stream), "gram_model_build_token_tables")
        keep.append(tables)
        self._token_tables = tables

    def _get_workspace(self, handle, B, N, L, K, max_length) -> torch.Tensor:
        lib = _lib.load()
        need = lib.gram_workspace_bytes(handle, B, N, L, K, max_length)
        if need < 0:
            raise _lib.GramHipError(
                f"unsupported problem size B={B} N={N} L={L} K={K} max_length={max_length} "
                f"(N <= max_item_num+1, L <= {self._max_passage_len}, N*L <= {self._max_fused_tokens}, K <= 64, max_length <= {_lib.GRAM_MAX_DEC_LEN}; "
                f"the Trie's fan-out is not limited)"
            )
        return self._ensure_workspace(need)

    def _tail_workspace(self, handle, B, N, L, K, max_length, steps) -> Optional[torch.Tensor]:
        """The workspace of a tail-pass call (gram_workspace_bytes_tail), or None where the device cannot hold it: the call then
        decodes step by step on the step-wise workspace.  The current workspace is given up only when the larger one is known to
        fit -- what the driver reports free, plus what PyTorch's allocator holds unused, plus the current workspace itself, less a
        margin -- and a shape that did not fit is remembered (with a one-time warning), so that a runner whose batch was sized without
        the forest's rows does not free and re-allocate most of the HBM on every call."""
        key = (int(handle), B, N, L, K, max_length, steps)
        if key in self._tail_no_fit:
            return None
        dev = self._device()
        need = int(_lib.load().gram_workspace_bytes_tail(handle, B, N, L, K, max_length, steps))
        if need <= 0:
            return None
        cur = self._workspace if self._workspace is not None and self._workspace.device == dev else None
        if cur is not None and cur.numel() >= need:
            return cur
        free, _total = torch.cuda.mem_get_info(dev)
        unused = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        room = free + unused + (cur.numel() if cur is not None else 0)
        if need + self._TAIL_FIT_MARGIN <= room:
            try:
                return self._ensure_workspace(need)
            except torch.cuda.OutOfMemoryError:
                pass
        self._tail_no_fit.add(key)
        import warnings
        warnings.warn(f"generate: the tail pass needs a workspace of {need / 2**30:.1f} GiB at B={B}, which does not fit this device "
                      f"next to what it holds; decoding step by step (size the batch with max_users_per_call(..., "
                      f"prefix_allowed_tokens_fn=fn))")
        return None

    _TAIL_FIT_MARGIN = 512 * 2**20  # (outputs and small temporaries of the call itself)

    def _ensure_workspace(self, need: int) -> torch.Tensor:
        dev = self._device()
        if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
            self._workspace = None
            torch.cuda.empty_cache()  # hand the old workspace (and whatever else the caching allocator holds unused) back first:
            #                           the new one is most of the HBM, and the allocator does not always manage that by itself
            self._workspace = torch.empty(int(need), dtype=torch.uint8, device=dev)
        return self._workspace

    def _tail_plan(self, fn, K: int, max_length: int, filtered: bool = False):
        """(d_tail, steps) of the Trie behind ``fn`` where a ``generate`` of this kind can take the tail pass (gram_generate_tail) at
        some batch size, else (0, 0): beam search on a Trie closure, no item filters, the short cross-attention, a tail inside the
        call's steps.  Whether a given batch takes it is gram_tail_pass_wanted's answer for that shape."""
        if fn is None or K <= 1 or filtered or self._max_fused_tokens > _lib.GRAM_MAX_FUSED_LEN or self._closure_trie(fn) is None:
            return 0, 0
        _sub, d_tail, steps = self._flat_trie(fn).tail_tables()
        if not (2 <= d_tail < int(max_length) and 1 <= steps <= _lib.GRAM_TAIL_MAX_STEPS):
            return 0, 0
        return d_tail, steps

    def _generate_bytes(self, handle, B: int, N: int, Lp: int, K: int, max_length: int, tail_steps: int) -> int:
        """workspace of one ``generate``: gram_workspace_bytes, or gram_workspace_bytes_tail where the call would take the tail pass"""
        lib = _lib.load()
        if tail_steps > 0 and lib.gram_tail_pass_wanted(handle, B, N, Lp) == 1:
            return int(lib.gram_workspace_bytes_tail(handle, B, N, Lp, K, max_length, tail_steps))
        return int(lib.gram_workspace_bytes(handle, B, N, Lp, K, max_length))

    def max_users_per_call(self, N: int, L: int, K: int, max_length: int, limit: int = 4096, headroom: float = 0.9,
                           prefix_allowed_tokens_fn: Optional[Callable] = None) -> int:
        """Largest batch B <= limit whose ``generate`` workspace fits the device's free HBM: what the runners size their GPU batches
        with, whatever ``--eval_batch_size`` the loader was built with (results do not depend on the batch a user is scored in).
        With ``prefix_allowed_tokens_fn`` (the Trie closure the calls will search) the workspace is the one those calls ask for: where
        the Trie has a tail and a batch is large enough to take the tail pass, gram_workspace_bytes_tail (the forest's rows, about a
        tenth more) -- a batch sized without them would never fit the pass and decode step by step.  Memory held by this model's
        current workspace counts as free (it is re-used or replaced); the handle's token tables (_build_token_tables) are allocated
        by the time the free memory is read, so they are already subtracted."""
        self._check_fused_len(N, L)
        handle = self._pack()
        lib = _lib.load()
        dev = self._device()
        Lp = (int(L) + 31) // 32 * 32
        torch.cuda.empty_cache()  # unused blocks of PyTorch's caching allocator go back to the driver first (once per evaluation)
        free, _total = torch.cuda.mem_get_info(dev)
        if self._workspace is not None and self._workspace.device == dev:
            free += self._workspace.numel()
        budget = int(free * headroom)
        lo, hi = 1, max(1, int(limit))
        steps = self._tail_plan(prefix_allowed_tokens_fn, K, max_length)[1]
        if 0 <= self._generate_bytes(handle, hi, N, Lp, K, max_length, steps) <= budget:
            return hi
        while lo < hi:  # workspace bytes grow monotonically with B (the tail's bytes come in at the size rule's batch and stay)
            mid = (lo + hi + 1) // 2
            need = self._generate_bytes(handle, mid, N, Lp, K, max_length, steps)
            if 0 <= need <= budget:
                lo = mid
            else:
                hi = mid - 1
        return lo

    @staticmethod
    def _closure_trie(fn: Callable):
        for cell in getattr(fn, "__closure__", None) or ():
            obj = cell.cell_contents
            if isinstance(obj, Trie):  # (checked first: reading `trie_dict` of a gram_amd Trie builds its nested dict)
                return obj
            if hasattr(obj, "trie_dict") and hasattr(obj, "get"):  # the reference's own utils.generation_trie.Trie
                return obj
        return None

    def _flat_trie(self, fn: Callable) -> FlatTrie:
        """Device CSR of the closure's Trie, cached per Trie OBJECT.  The entry holds a strong reference to its
        source, so the id cannot be recycled by a later Trie while the entry is alive (the runner builds a fresh
        Trie per evaluation), and the item count guards against in-place ``add`` calls."""
        trie = self._closure_trie(fn)
        cached = self._tries.get(id(trie))
        if cached is None or cached[0] is not trie or cached[1].n_sequences != len(trie):
            cached = (trie, FlatTrie(trie))
            self._tries = {id(trie): cached}  # one live Trie per eval; drop stale ones
        return cached[1]

    # ------------------------------------------------------------------ which passages the encoder runs on
    _CACHE_L = _lib.GRAM_MAX_PASSAGE_LEN  # row length of the passage cache: the model's set_max_passage_len
    _KEY_MULT: Dict[tuple, torch.Tensor] = {}  # (device, width) -> multipliers

    @staticmethod
    def _canonical(rows_ids: torch.Tensor, rows_mask: torch.Tensor, width: int = _lib.GRAM_MAX_PASSAGE_LEN) -> torch.Tensor:
        """(P, width) int32: token id where valid, -1 elsewhere -- the identity of a passage (position-wise).  ``width`` is the
        cache's row length and never below the rows' own (a negative pad would cut tokens off: two passages that differ only
        behind the cut would then share an identity)."""
        canon = torch.where(rows_mask.bool(), rows_ids, rows_ids.new_full((), -1)).to(torch.int32)
        if canon.shape[1] > width:
            raise ValueError(f"passages of {canon.shape[1]} tokens do not fit the passage cache's rows of {width}")
        return torch.nn.functional.pad(canon, (0, width - canon.shape[1]), value=-1)

    @staticmethod
    def _passage_keys(canon: torch.Tensor) -> torch.Tensor:
        # 64-bit key over the row's own width, overflow-free ((id+1) < 2^15, multiplier < 2^31, at most 512 = 2^9 terms: the sum
        # stays below 2^55 < 2^63); a key match is always confirmed against the stored tokens, so a collision costs a miss, never a
        # wrong hit
        width = int(canon.shape[1])
        mult = GRAM._KEY_MULT.get((canon.device, width))
        if mult is None:
            g = torch.Generator().manual_seed(0x6772616D)
            mult = torch.randint(1, 2 ** 31 - 1, (width,), generator=g, dtype=torch.int64).to(canon.device)
            GRAM._KEY_MULT[(canon.device, width)] = mult
        return ((canon.to(torch.int64) + 1) * mult).sum(dim=1)

    # The passage cache: x f32 [capacity][_CACHE_L][d] (the encoder's residual stream before the final norm), canon i32 [capacity][_CACHE_L]
    # (the tokens: the identity of a passage), n rows in use, keys (sorted) / perm over the rows in use.
    def _pcache_rows(self, n_new: int):
        """Make room for n_new more passages; returns (cache dict, first new row).  The buffers grow geometrically (a dataset's item
        prompts arrive over several batches; `reserve_passage_cache` sizes them once)."""
        dev, d = self._device(), self.config.d_model
        pc = self._pcache
        used = 0 if pc is None else pc["n"]
        cap = 0 if pc is None else pc["x"].shape[0]
        if used + n_new > cap:
            new_cap = max(used + n_new, 2 * cap, int(getattr(self, "_pcache_reserve", 0)))
            x = torch.empty(new_cap, self._CACHE_L, d, dtype=torch.float32, device=dev)
            canon = torch.full((new_cap, self._CACHE_L), -1, dtype=torch.int32, device=dev)
            if used:
                x[:used].copy_(pc["x"][:used])
                canon[:used].copy_(pc["canon"][:used])
            pc = dict(x=x, canon=canon, n=used, keys=None if pc is None else pc["keys"], perm=None if pc is None else pc["perm"])
            self._pcache = pc
        return pc, used

    def _pcache_commit(self, pc, n_total: int) -> None:
        keys = self._passage_keys(pc["canon"][:n_total])
        pc["keys"], pc["perm"] = torch.sort(keys, stable=True)
        pc["n"] = n_total

    def reserve_passage_cache(self, n_passages: int) -> None:
        """Capacity hint: the number of distinct passages that will be cached (a dataset's item count)."""
        self._pcache_reserve = int(n_passages)

    def set_passage_harvest(self, on: bool = True, first_slot: int = 1) -> None:
        """With harvesting on, every passage a ``generate`` call had to encode in a slot >= first_slot joins the passage cache when
        the call returns -- its residual-stream rows are still in the workspace (gram_workspace_encoder_x_offset), nothing is
        encoded twice -- so an evaluation needs no separate cache-fill pass: a batch pays for the item prompts it is the first to
        see and the later ones find them.  Slot 0 is the user's own prompt (test_dataset_gram.py:203-210), never seen again.
        Results do not change (the cache is result-neutral bit for bit)."""
        self._harvest = bool(on)
        self._harvest_first_slot = int(first_slot)

    @torch.no_grad()
    def cache_passages(self, input_ids, attention_mask, chunk: int = 1024) -> int:
        """Pre-encode user-independent passages.

        A GRAM input is passage 0 = the user prompt plus up to ``max_item_num`` ITEM prompts
        (test_dataset_gram.py:115-123,203-210); EncoderWrapper.forward (gram.py:200-256) encodes every passage on
        its own and adds the slot's position embedding afterwards, so an item prompt's encoder states are the same
        for every user and every slot.  Passages registered here (``(P, L)`` or ``(B, N, L)`` ids + mask, e.g. all
        item prompts of the dataset) are encoded once; ``generate`` then recognises them by their tokens and runs the
        encoder only on the rest.  Results are bit-identical with and without the cache.  The cache holds the fp32
        residual stream (max passage length x d_model x 4 B per passage) on the device and is dropped whenever the weights change.
        Returns the number of passages cached so far."""
        handle = self._pack()
        lib = _lib.load()
        dev = self._device()
        ids = input_ids.to(dev, torch.int64).reshape(-1, input_ids.shape[-1])
        mask = attention_mask.to(dev).reshape(-1, attention_mask.shape[-1]).ne(0)
        if ids.shape != mask.shape or ids.shape[1] > self._CACHE_L:
            raise ValueError(f"passages must be (P, L <= {self._CACHE_L}) ids with a mask of the same shape")
        keep = mask.any(dim=1)
        canon = self._canonical(ids[keep], mask[keep], self._CACHE_L)
        canon = canon[self._first_unseen(canon)]
        n_new = int(canon.shape[0])
        if n_new == 0:
            return 0 if self._pcache is None else int(self._pcache["n"])
        full_ids = canon.clamp(min=0).to(torch.int64).contiguous()
        full_mask = canon.ge(0).view(torch.uint8).contiguous()
        pc, base = self._pcache_rows(n_new)
        pc["canon"][base:base + n_new] = canon
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for lo in range(0, n_new, chunk):
                n = min(chunk, n_new - lo)
                ws = self._get_workspace(handle, n, 1, self._CACHE_L, 1, 2)
                _lib.check(lib.gram_encode_passages(handle, full_ids[lo:lo + n].data_ptr(), full_mask[lo:lo + n].data_ptr(), n,
                                                    self._CACHE_L, ws.data_ptr(), ws.numel(), pc["x"][base + lo:base + lo + n].data_ptr(),
                                                    stream), "gram_encode_passages")
        self._pcache_commit(pc, base + n_new)
        return base + n_new

    def clear_passage_cache(self) -> None:
        self._pcache = None

    def _first_unseen(self, canon: torch.Tensor) -> torch.Tensor:
        """bool [P]: the first occurrence of every passage of `canon` that the cache does not hold yet."""
        keys = self._passage_keys(canon)
        order = torch.argsort(keys, stable=True)
        first = torch.ones_like(keys, dtype=torch.bool)
        first[order[1:]] = keys[order[1:]] != keys[order[:-1]]
        if self._pcache is not None and self._pcache["n"] > 0:
            first &= self._lookup(canon, keys)[0].logical_not()
        return first

    def _lookup(self, canon: torch.Tensor, keys: torch.Tensor):
        pc = self._pcache
        pos = torch.searchsorted(pc["keys"], keys).clamp(max=pc["keys"].numel() - 1)
        slot = pc["perm"][pos]
        hit = (pc["keys"][pos] == keys) & (pc["canon"].index_select(0, slot) == canon).all(dim=1)
        return hit, slot

    def _plan_encoder(self, ids, mask, B, N, Lp):
        """gram_compaction_t for this batch as (struct, keep-alive list, tensors), or None when the encoder simply runs on all B*N passages."""
        return self._plan(ids, mask, B, N, Lp)[0]

    @staticmethod
    def _comp_args(comp) -> tuple:
        """The seven comp_* / cache_* arguments of the whole-path ops (gram_amd/ops.py) from ``_plan``'s compaction, or None for off."""
        if not comp:
            return None, None, None, None, None, 0, 0
        t = comp[2]
        return t["comp_map"], t["comp_ids"], t["comp_mask"], t["cache_slot"], t["cache_x"], int(t["n_cached"]), int(t["cache_L"])

    def _plan(self, ids, mask, B, N, Lp):
        """(gram_compaction_t for this batch -- or None when the encoder simply runs on all B*N passages --, harvest plan or None).

        Ragged batches: the Collator pads every user to the batch's largest passage count with fully masked passages
        (Collator.py:410-436); the encoder skips them.  Passages found in the passage cache skip it too.  One small
        D2H sync for the counts; the gathers are input plumbing.  GRAM_COMPACT=0 disables both.
        Harvest plan (set_passage_harvest): (compact rows of the passages to add to the cache after the call, their tokens)."""
        harvest = bool(getattr(self, "_harvest", False)) and N > int(getattr(self, "_harvest_first_slot", 1))
        have = self._pcache is not None and self._pcache["n"] > 0
        if os.environ.get("GRAM_COMPACT", "1") == "0" or (N == 1 and not have):
            return None, None
        rows_ids, rows_mask = ids.view(B * N, Lp), mask.view(B * N, Lp)
        active = rows_mask.ne(0).any(dim=1)
        canon = self._canonical(rows_ids, rows_mask, self._CACHE_L) if (have or harvest) else None
        if have:
            hit, slot = self._lookup(canon, self._passage_keys(canon))
            hit &= active
        else:
            hit = torch.zeros_like(active)
        miss = active & ~hit
        n_miss, n_hit, users = torch.stack([miss.sum(), hit.sum(), active.view(B, N).any(dim=1).sum()]).tolist()
        if users < B:
            raise ValueError("every user needs at least one passage with a valid token")
        plan = None
        if harvest and n_miss:
            # misses in slots >= first_slot, one per distinct passage; compact row of flat passage f = its rank among the misses
            slot_ok = (torch.arange(B * N, device=ids.device) % N) >= self._harvest_first_slot
            cand = (miss & slot_ok).nonzero().squeeze(1)
            if cand.numel():
                c_canon = canon.index_select(0, cand)
                cand = cand[self._first_unseen(c_canon)]
                rank = torch.cumsum(miss.to(torch.int64), 0) - 1
                plan = (rank.index_select(0, cand), canon.index_select(0, cand))
        if n_hit == 0 and n_miss == B * N:
            return None, plan
        midx, hidx = miss.nonzero().squeeze(1), hit.nonzero().squeeze(1)
        c_ids = rows_ids.index_select(0, midx).contiguous()
        c_mask = rows_mask.index_select(0, midx).contiguous()
        c_map = torch.cat([midx, hidx]).to(torch.int32).contiguous()
        keep = [c_ids, c_mask, c_map]
        comp = _lib.Compaction(n_miss + n_hit, c_map.data_ptr(), c_ids.data_ptr(), c_mask.data_ptr(), 0, 0, None, None)
        tens = dict(comp_map=c_map, comp_ids=c_ids, comp_mask=c_mask, cache_slot=None, cache_x=None, n_cached=0, cache_L=0)
        if n_hit:
            slots = slot.index_select(0, hidx).to(torch.int32).contiguous()
            keep += [slots, self._pcache["x"]]
            comp.n_cached, comp.cache_L = n_hit, self._CACHE_L
            comp.cache_x, comp.cache_slot = self._pcache["x"].data_ptr(), slots.data_ptr()
            tens.update(cache_slot=slots, cache_x=self._pcache["x"], n_cached=n_hit, cache_L=self._CACHE_L)
        return (comp, keep, tens), plan

    def _harvest_from_workspace(self, plan, ws, handle, B, N, Lp, K, max_length) -> None:
        """Add the planned passages to the cache from the residual stream the generate() call left in the workspace."""
        rows, canon = plan
        n_new = int(rows.numel())
        if n_new == 0:
            return
        d = self.config.d_model
        off = _lib.load().gram_workspace_encoder_x_offset(handle, B, N, Lp, K, max_length)
        if off < 0:
            raise _lib.GramHipError("gram_workspace_encoder_x_offset rejected the shape")
        wx = ws[off: off + B * N * Lp * d * 4].view(torch.float32).view(B * N, Lp, d)
        pc, base = self._pcache_rows(n_new)
        dst = pc["x"][base:base + n_new]
        torch.index_select(wx, 0, rows, out=dst[:, :Lp])
        if Lp < self._CACHE_L:
            dst[:, Lp:].zero_()  # positions past the batch's L are padding for these passages (gram_compaction_t.cache_L semantics)
        pc["canon"][base:base + n_new] = canon
        self._pcache_commit(pc, base + n_new)

    # ------------------------------------------------------------------ the hot path
    @torch.no_grad()
    def generate(self, input_ids, attention_mask, max_length, prefix_allowed_tokens_fn=None, num_beams=1,
                 num_return_sequences=None, output_scores=True, return_dict_in_generate=True, length_penalty=1.0,
                 exclude_items=None, allowed_items=None, candidates=None, do_sample=False, temperature=1.0, top_k=50, top_p=1.0,
                 uniforms=None, generator=None, num_beam_groups=1, diversity_penalty=0.0, replacement=True, seed=None,
                 user_keys=None, item_bias=None, bias_lookahead=True, item_mask=None, **unused):
        """GRAM.generate (gram.py:74-107) with the kwargs single_runner_gram.py:641-651 passes.

        input_ids (B,N,L) int64, attention_mask (B,N,L) bool on the model's device.  Returns a
        mapping with ``sequences`` (B*num_return_sequences, T) int64 -- user-major, best first,
        0-padded, starting with the decoder start token -- and ``sequences_scores`` (fp32).

        Per-user item filters: ``exclude_items`` (what a user must not get, e.g. its history) or ``allowed_items`` (the only items
        a user may get, e.g. a retrieval stage's output) -- one of the two, a (B, M) integer tensor padded with -1 or B Python
        lists of indices into ``candidates``, the token sequences the closure's Trie was built from (the list ``sequence_items``
        takes; required with either).  User b then gets exactly what this call returns for that user alone with
        ``prefix_allowed_tokens_fn(Trie(A_b))``, A_b its remaining candidates, bit for bit -- the search walks a per-user view of
        the one shared device Trie.  Two candidates that spell the same sequence share a Trie leaf: naming
        either names the sequence.  At most 4096 entries per user (larger sets: ``item_mask``, below); a user left without any
        item is a ``ValueError``.

        Sampling: ``do_sample=True`` (with ``num_beams=1``) draws ``num_return_sequences`` = R <= 64 items per user from
        p(item | user) restricted to the Trie -- HF 4.26's ``sample``: the Trie mask, then ``temperature`` (> 0), ``top_k`` (None =
        HF's default 50, 0 = off) and ``top_p`` (in (0, 1]) on the raw logits of the row's Trie children, then one draw (DESIGN.md
        section 4.8).  The draw is inverse-CDF sampling from ``uniforms``, float32 (B, R, max_length - 1) in [0, 1) on any device --
        row (b, r) takes the first kept child whose cumulative weight exceeds ``uniforms[b, r, t]`` times the total at step t --
        or, without it, from ``torch.rand(..., generator=generator)`` on the model's device.  That is the same DISTRIBUTION as HF's
        ``torch.multinomial``, not the same draw for a given torch seed.  Returns ``sequences`` (B*R, width) user-major,
        ``sequences_scores=None`` (as HF's ``sample``), ``sequence_logprobs`` (B*R,) = the model's log-probability of each row (what
        ``score_sequences`` returns for it) and ``sample_logprobs`` (B*R,) = its log-probability under the warped distribution it was
        drawn from.  ``exclude_items`` / ``allowed_items`` work as for beam search.  A row's draw depends on its user, its uniforms and
        the parameters only, not on the batch or on R.  Without ``do_sample`` the five sampling arguments are ignored, as before.

        Sampling WITHOUT replacement: ``do_sample=True, replacement=False`` returns ``num_return_sequences`` = R <= 64 DISTINCT items
        per user, in the order of sampling without replacement (Plackett-Luce) from p(item | user) restricted to the Trie at
        ``temperature`` -- stochastic beam search (Kool et al. 2019): a slate for exploration traffic,
        negatives, or importance-weighted estimators over the catalogue.  ``top_k`` (other than None / 0 / the default 50, which is
        not applied) and ``top_p`` < 1 are a ``NotImplementedError`` -- truncation together with exact without-replacement sampling
        is not defined here -- and ``uniforms=`` is a ``ValueError``: the randomness is counter-based, a function of ``seed`` (an
        int; without it one int64 is drawn from ``generator`` or the global torch RNG on the CPU), the user's entry of ``user_keys``
        ((B,) int64, default ``arange(B)``) and the token prefix.  Pass STABLE user ids as ``user_keys``: a user's draw then does not
        depend on its place in the batch, on the batch's other users or on R (the rows of R' < R are the first R' rows of R).
        Returns ``sequences`` (B*R, width) user-major, largest perturbed score first, ``sequences_scores=None``,
        ``sequence_logprobs`` (the model's, as above), ``sample_logprobs`` (each item's log-probability under the Trie-renormalised
        distribution) and ``perturbed_scores`` (its Gumbel-perturbed log-probability G; the R-th largest is the threshold of the
        importance weights).  A user with fewer than R items (``exclude_items`` / ``allowed_items`` work as for sampling) gets rows
        of the start token followed by padding with -inf in all three, and no error.

        Group (diverse) beam search: ``num_beam_groups`` = G > 1, a divisor of ``num_beams``, with ``diversity_penalty`` >= 0 -- HF
        4.26's ``group_beam_search`` with the Hamming diversity penalty: the beams are G groups searched one
        after the other in every step, and a token costs a group ``diversity_penalty`` for every beam of the earlier groups that
        chose it in that step, which spreads a user's list over different branches of the Trie.  Returns ``sequences`` and
        ``sequences_scores`` as beam search does; the scores include the penalties, as in HF.  The penalty acts per step, not per
        sequence, so two groups can return the SAME sequence: ``sequence_items`` then maps both rows to the same item.
        ``exclude_items`` / ``allowed_items`` work as for beam search.  G = 1 is plain beam search (and refuses a non-zero
        ``diversity_penalty``, as before).

        Per-item score biases: ``item_bias`` = T, a finite float32 tensor on any device of shape (len(candidates),) -- one bias per
        item, shared by all users -- or (B, len(candidates)), with ``num_beams`` >= 2 and ``candidates`` as for the item filters
        (DESIGN.md section 4.11): boosts and demotions, a popularity correction, a soft penalty for seen items, a second model's
        scores.  The search runs on log p + T: a returned item's ``sequences_scores`` is (its sum of log-probabilities +
        T[item]) / length^length_penalty up to fp32 rounding, and the list is the one beam search finds for that score -- not a
        re-ranking of the unbiased list.  Two candidates that spell one sequence share a leaf: the bias of the first counts.  With
        ``bias_lookahead=True`` (the default) every step already sees the best bias still reachable below a Trie node (each edge adds
        the difference of the two nodes' potentials, which telescopes to T[item] at the leaf), so a boosted item is not pruned
        before its last token and the running scores never rise along a path; ``False`` adds each bias at its item's last token
        only.  A beam cut off by a ``max_length`` shorter than its item carries the optimistic potential of its node.  Biased calls
        decode step by step (no tail pass).  ``exclude_items`` / ``allowed_items`` compose: the look-ahead is taken over the shared
        Trie and ignores them, the returned scores do not change.  The potentials are a float32 (rows, n_nodes) tensor with rows = 1
        or B, allocated per call NEXT TO the workspace: ``max_users_per_call`` does not know of it (n_nodes * 4 bytes per user with
        a per-user bias).  ``do_sample=True``, ``num_beam_groups`` > 1, ``num_beams`` = 1 and the callback form of
        ``prefix_allowed_tokens_fn`` are a ``NotImplementedError``.  ``bias_lookahead`` is ignored without ``item_bias``.

        Per-user item masks: ``item_mask`` = M, a (B, len(candidates)) tensor of dtype bool, uint8 or any integer type, on any device
        and of any strides, with ``candidates`` as for the item filters: M[b, i] != 0 says user b may get
        candidate i.  The semantics are ``allowed_items``' with the same sets -- user b gets, bit for bit, what it gets alone with
        ``prefix_allowed_tokens_fn(Trie(A_b))`` -- but a set may have ANY size (the lists stop at 4096 entries per user), every user
        has its own, and filters compose with torch on the device: ``cat_mask[cat] & ~seen & in_stock``.  Works with beam search
        (``num_beams`` >= 2) and greedy search (``num_beams=1``) in every precision mode; masked calls decode step by step (no tail
        pass).  Two candidates that spell one sequence share a leaf, which is kept iff M keeps either.  A user's set travels as a
        bitset over the Trie's leaves with a running count beside every word; these records are allocated per call NEXT TO the
        workspace, B * (n_leaves / 32 + 1) * 8 bytes, and ``max_users_per_call`` does not count them.  A wrong shape or dtype, a
        missing ``candidates``, the callback form of ``prefix_allowed_tokens_fn``, ``item_mask`` together with ``exclude_items`` /
        ``allowed_items`` (fold those into the mask) and a user whose row keeps nothing are a ``ValueError``; ``item_mask`` with
        ``do_sample=True``, ``num_beam_groups`` > 1 or ``item_bias`` is a ``NotImplementedError``."""
        if prefix_allowed_tokens_fn is None:
            raise NotImplementedError("unconstrained generation is not on GRAM's scoring path (a Trie is always passed)")
        # HF kwargs that would change the search: refuse the ones this path does not implement instead of ignoring them
        neutral = {"do_sample": False, "early_stopping": False, "num_beam_groups": 1, "repetition_penalty": 1.0,
                   "no_repeat_ngram_size": 0, "diversity_penalty": 0.0, "use_cache": True, "temperature": 1.0, "top_k": 50,
                   "top_p": 1.0, "min_length": 0, "pad_token_id": 0, "eos_token_id": 1, "decoder_start_token_id": 0}
        G = 1 if num_beam_groups is None else int(num_beam_groups)
        if G == 1:  # (one group is the plain search: the two arguments are judged by name like every other HF keyword)
            unused = dict(unused, num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)
        else:  # (every refusal of the group search, before anything touches the device)
            lam = self._group_args(int(num_beams), G, diversity_penalty, do_sample, prefix_allowed_tokens_fn, num_return_sequences)
        if not do_sample:  # (greedy and beam search ignore the sampling arguments, by name as they always did)
            unused = dict(unused, **{k: v for k, v in (("uniforms", uniforms), ("generator", generator), ("seed", seed),
                                                       ("user_keys", user_keys)) if v is not None})
            if not replacement:
                unused = dict(unused, replacement=replacement)
        elif replacement:
            unused = dict(unused, **{k: v for k, v in (("seed", seed), ("user_keys", user_keys)) if v is not None})
        for k, v in unused.items():
            if k in neutral:
                if v is not None and v != neutral[k] and k not in ("temperature", "top_k", "top_p"):
                    raise NotImplementedError(f"generate({k}={v!r}) is not supported by the HIP scoring path "
                                              f"(only {k}={neutral[k]!r}, the value the GRAM runners use)")
            elif v is not None:
                import warnings
                warnings.warn(f"gram_amd.GRAM.generate ignores the keyword argument {k!r}")
        if input_ids.dim() != 3:
            raise ValueError("input_ids must be (B, N, L)")
        masked = item_mask is not None
        if masked:  # (every refusal of the masked search that needs no device, before anything touches one)
            item_mask = self._mask_args(item_mask, input_ids.shape[0], G, do_sample, prefix_allowed_tokens_fn, candidates,
                                        exclude_items is not None or allowed_items is not None, item_bias is not None)
        biased = item_bias is not None
        if biased:  # (every refusal of the biased search, before anything touches the device)
            item_bias = self._bias_args(item_bias, input_ids.shape[0], int(num_beams), G, do_sample, prefix_allowed_tokens_fn, candidates)
        if do_sample:  # (every refusal of the sampling path, before anything touches the device)
            sampling = self._sample_args(input_ids.shape[0], int(max_length), num_beams, num_return_sequences, temperature, top_k, top_p,
                                         uniforms, prefix_allowed_tokens_fn)
            if not replacement:
                seed, user_keys = self._distinct_args(input_ids.shape[0], top_k, top_p, uniforms, seed, user_keys, generator)
        self._check_passage_len(input_ids.shape[-1])
        self._check_fused_len(input_ids.shape[1], input_ids.shape[2])
        handle = self._pack()
        lib = _lib.load()
        dev = self._device()
        K = int(num_beams)
        nret = int(num_return_sequences or K)
        B, N, L = input_ids.shape
        ids = input_ids.to(dev, torch.int64)
        mask = attention_mask.to(dev).ne(0).view(torch.uint8) if attention_mask.dtype != torch.bool else attention_mask.to(dev).view(torch.uint8)
        Lp = (L + 31) // 32 * 32  # masked padding is invisible to attention: pad L to the kernel tile
        if Lp != L:
            ids = torch.nn.functional.pad(ids, (0, Lp - L))
            mask = torch.nn.functional.pad(mask, (0, Lp - L))
        ids, mask = ids.contiguous(), mask.contiguous()
        filtered = exclude_items is not None or allowed_items is not None
        if exclude_items is not None and allowed_items is not None:
            raise ValueError("generate: exclude_items and allowed_items are mutually exclusive")
        if filtered and candidates is None:
            raise ValueError("generate: exclude_items / allowed_items index `candidates` (the sequences the Trie was built from): pass it")
        if filtered and self._closure_trie(prefix_allowed_tokens_fn) is None:
            raise ValueError("generate: exclude_items / allowed_items need the Trie closure form of prefix_allowed_tokens_fn "
                             "(an arbitrary callback receives batch_id and can filter per user itself)")
        if self._closure_trie(prefix_allowed_tokens_fn) is None:
            if K == 1:
                raise NotImplementedError("greedy search needs the Trie closure form of prefix_allowed_tokens_fn")
            return self._generate_with_callback(ids, mask, B, N, Lp, K, nret, int(max_length), float(length_penalty),
                                                prefix_allowed_tokens_fn, return_dict_in_generate)
        flat = self._flat_trie(prefix_allowed_tokens_fn)
        if filtered:  # (validated before anything below touches the passage cache or the workspace)
            allow = allowed_items is not None
            items = self._user_item_lists(allowed_items if allow else exclude_items, allow, B, flat, candidates, dev)
        if masked:  # (as the lists: an empty user is refused before anything below touches the passage cache or the workspace)
            item_mask = self._user_item_mask(item_mask, flat, candidates, dev)
        comp, harvest_plan = self._plan(ids, mask, B, N, Lp)
        _ctrie, (t_off, t_tok, t_node) = flat.to_device(dev)
        if do_sample and not replacement:
            # stochastic beam search: ONE custom op over the C ABI (gram_amd/ops.py -> gram_generate_sbs / gram_generate_sbs_items)
            R, tau = sampling[:2]
            need = int(lib.gram_workspace_bytes_sbs(handle, B, N, Lp, R, int(max_length), int(flat.max_fanout)))
            if need < 0:
                raise _lib.GramHipError(f"unsupported problem size B={B} N={N} L={Lp} num_return_sequences={R} max_length={max_length}")
            ws = self._ensure_workspace(need)
            from .. import ops as _ops  # noqa: F401  (registers torch.ops.gram.*)
            args = (ids, mask, int(handle), ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len), R, int(max_length),
                    tau, seed, user_keys.to(dev).contiguous(), *self._comp_args(comp))
            if filtered:
                leaf_lo, leaf_hi = flat.leaf_ranges_on(dev)
                out = torch.ops.gram.sample_distinct_items(*args, leaf_lo, leaf_hi, flat.item_ranks_on(dev, candidates)[1], items, allow)
            else:
                out = torch.ops.gram.sample_distinct(*args)
            seqs, model_lp, sample_lp, perturbed, width = out
            if harvest_plan is not None:
                self._harvest_from_workspace(harvest_plan, ws, handle, B, N, Lp, R, int(max_length))
            seqs = seqs[:, : int(width[0])]
            if not return_dict_in_generate:
                return seqs
            return GenerateOutput(sequences=seqs, sequences_scores=None, sequence_logprobs=model_lp, sample_logprobs=sample_lp,
                                  perturbed_scores=perturbed)
        if do_sample:
            # HF's sample on the Trie: ONE custom op over the C ABI (gram_amd/ops.py -> gram_sample / gram_sample_items)
            R, tau, k_top, p_top = sampling
            need = int(lib.gram_workspace_bytes_sample(handle, B, N, Lp, R, int(max_length), int(flat.max_fanout)))
            if need < 0:
                raise _lib.GramHipError(f"unsupported problem size B={B} N={N} L={Lp} num_return_sequences={R} max_length={max_length}")
            ws = self._ensure_workspace(need)
            if uniforms is None:
                shape = (B, R, int(max_length) - 1)
                gdev = generator.device if generator is not None else dev
                uniforms = torch.rand(shape, generator=generator, dtype=torch.float32, device=gdev)
            uni = uniforms.detach().to(dev).contiguous()
            from .. import ops as _ops  # noqa: F401  (registers torch.ops.gram.*)
            args = (ids, mask, int(handle), ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len), R, int(max_length),
                    tau, k_top, p_top, uni, *self._comp_args(comp))
            if filtered:
                leaf_lo, leaf_hi = flat.leaf_ranges_on(dev)
                seqs, model_lp, sample_lp, width = torch.ops.gram.sample_items(*args, leaf_lo, leaf_hi,
                                                                                flat.item_ranks_on(dev, candidates)[1], items, allow)
            else:
                seqs, model_lp, sample_lp, width = torch.ops.gram.sample(*args)
            if harvest_plan is not None:
                self._harvest_from_workspace(harvest_plan, ws, handle, B, N, Lp, R, int(max_length))
            seqs = seqs[:, : int(width[0])]
            if not return_dict_in_generate:
                return seqs
            return GenerateOutput(sequences=seqs, sequences_scores=None, sequence_logprobs=model_lp, sample_logprobs=sample_lp)
        # the tail pass (gram_generate_tail; taken by size, GRAM_TAIL_PASS=0 switches it off: gram_tail_pass_wanted): where the Trie has a tail inside this call's
        # steps, the workspace grows by the forest's rows (gram_workspace_bytes_tail); a device that cannot hold them decodes step by
        # step -- the same results
        d_tail, tail_steps = self._tail_plan(prefix_allowed_tokens_fn, K, int(max_length), filtered or masked) if G == 1 and not biased else (0, 0)
        tail = tail_steps > 0 and _lib.load().gram_tail_pass_wanted(handle, B, N, Lp) == 1
        ws = self._tail_workspace(handle, B, N, Lp, K, int(max_length), tail_steps) if tail else None
        tail = ws is not None
        if ws is None:
            ws = self._get_workspace(handle, B, N, Lp, K, int(max_length))
        if K == 1 and nret != 1:
            raise ValueError("num_return_sequences must be 1 for greedy search (num_beams == 1), as in HF generate")
        # the whole path is ONE PyTorch-ROCm custom op over the C ABI (gram_amd/ops.py -> gram_generate_ex / gram_generate_items)
        from .. import ops as _ops  # noqa: F401  (registers torch.ops.gram.*)
        args = (ids, mask, int(handle), ws, t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len), K, nret, int(max_length),
                float(length_penalty), *self._comp_args(comp))
        if G > 1:  # group beam search (gram_generate_groups): the same arguments, no tail pass
            lists = ()
            if filtered:
                lists = (*flat.leaf_ranges_on(dev), flat.item_ranks_on(dev, candidates)[1], items, allow)
            seqs, scores, width = torch.ops.gram.generate_groups(*args[:13], G, lam, *args[13:], *lists)
        elif biased:  # per-item score biases (gram_item_bias_table, then gram_generate_bias): the same arguments, no tail pass
            leaf_lo, leaf_hi = flat.leaf_ranges_on(dev)
            phi = torch.ops.gram.item_bias_table(item_bias.to(dev).contiguous(), flat.leaf_items_on(dev, candidates), leaf_lo, leaf_hi,
                                                 t_off, t_tok, t_node, int(flat.max_fanout), int(flat.min_seq_len),
                                                 0, bool(bias_lookahead))  # (0: the start token the search begins with)
            lists = (leaf_lo, leaf_hi, flat.item_ranks_on(dev, candidates)[1], items, allow) if filtered else ()
            seqs, scores, width = torch.ops.gram.generate_bias(*args[:13], phi, *args[13:], *lists)
        elif masked:  # per-user item masks (gram_user_mask_prepare, then gram_generate_mask): the same arguments, no tail pass
            leaf_lo, leaf_hi = flat.leaf_ranges_on(dev)
            seqs, scores, width, _kept = torch.ops.gram.generate_mask(*args, leaf_lo, leaf_hi, flat.leaf_items_on(dev, candidates),
                                                                      item_mask)
        elif filtered:
            leaf_lo, leaf_hi = flat.leaf_ranges_on(dev)
            seqs, scores, width = torch.ops.gram.generate_items(*args, leaf_lo, leaf_hi, flat.item_ranks_on(dev, candidates)[1], items,
                                                                allow)
        else:
            seqs, scores, width = torch.ops.gram.generate(*args, flat.tail_rows_on(dev) if tail else None, d_tail if tail else 0,
                                                          tail_steps if tail else 0)
        if harvest_plan is not None:
            self._harvest_from_workspace(harvest_plan, ws, handle, B, N, Lp, K, int(max_length))
        seqs = seqs[:, : int(width[0])]
        scores = scores if K > 1 else None  # num_beams == 1 is HF's greedy_search: it has no sequences_scores
        if not return_dict_in_generate:
            return seqs
        return GenerateOutput(sequences=seqs, sequences_scores=scores)

    def _group_args(self, K: int, G: int, diversity_penalty, do_sample, fn, num_return_sequences) -> float:
        """The arguments of ``generate(num_beam_groups=G > 1)``, or the refusal; returns the penalty.  Everything is checked on the
        host, before the model is packed or a tensor is moved."""
        if do_sample:
            raise ValueError("generate(num_beam_groups > 1) is a beam search: it does not go with do_sample=True (as in HF)")
        if G < 1 or G > K or K % G:
            raise ValueError(f"generate: num_beam_groups must be a divisor of num_beams (got num_beams={K}, num_beam_groups={G})")
        try:
            lam = float(0.0 if diversity_penalty is None else diversity_penalty)
        except (TypeError, ValueError):
            raise ValueError(f"generate: diversity_penalty must be a number (got {diversity_penalty!r})") from None
        if not (0.0 <= lam < float("inf")):
            raise ValueError(f"generate: diversity_penalty must be a finite number >= 0 (got {diversity_penalty!r}); 0.0 adds no penalty")
        if not 1 <= int(num_return_sequences or K) <= K:
            raise ValueError(f"generate: num_return_sequences must lie in [1, num_beams] (got {num_return_sequences!r})")
        if self._closure_trie(fn) is None:
            raise NotImplementedError("generate(num_beam_groups > 1) needs the Trie closure form of prefix_allowed_tokens_fn")
        return lam

    def _bias_args(self, item_bias, B: int, K: int, G: int, do_sample, fn, candidates) -> torch.Tensor:
        """The arguments of ``generate(item_bias=T)``, or the refusal; returns T as (rows, len(candidates)), rows = 1 or B.
        Everything is checked on the host, before the model is packed or a tensor is moved."""
        if do_sample:
            raise NotImplementedError("generate(item_bias=) is a beam search: biased sampling (do_sample=True) is not implemented")
        if G > 1:
            raise NotImplementedError("generate(item_bias=) with num_beam_groups > 1 is not implemented")
        if K == 1:
            raise NotImplementedError("generate(item_bias=) with num_beams=1 (greedy search) is not implemented: "
                                      "use num_beams=2, num_return_sequences=1")
        if self._closure_trie(fn) is None:
            raise NotImplementedError("generate(item_bias=) needs the Trie closure form of prefix_allowed_tokens_fn")
        if candidates is None:
            raise ValueError("generate: item_bias holds one bias per entry of `candidates` (the sequences the Trie was built from): pass it")
        n = len(candidates)
        if not isinstance(item_bias, torch.Tensor) or item_bias.dtype != torch.float32 or \
                tuple(item_bias.shape) not in ((n,), (B, n)) or n < 1:
            got = (tuple(item_bias.shape), item_bias.dtype) if isinstance(item_bias, torch.Tensor) else type(item_bias).__name__
            raise ValueError(f"generate: item_bias must be a float32 tensor of shape ({n},) = (len(candidates),) or ({B}, {n}) = "
                             f"(B, len(candidates)), got {got}")
        if not bool(torch.isfinite(item_bias).all()):
            raise ValueError("generate: item_bias must be finite (to rule an item out, use exclude_items)")
        return item_bias.detach().reshape(-1, n)

    def _mask_args(self, item_mask, B: int, G: int, do_sample, fn, candidates, filtered: bool, biased: bool) -> torch.Tensor:
        """The arguments of ``generate(item_mask=M)``, or the refusal; returns M detached.  Everything is checked on the host, before
        the model is packed or a tensor is moved (the one check that reads M's values, a user without any item, is
        ``_user_item_mask``'s)."""
        if do_sample:
            raise NotImplementedError("generate(item_mask=) with do_sample=True is not implemented (sampling takes exclude_items / allowed_items)")
        if G > 1:
            raise NotImplementedError("generate(item_mask=) with num_beam_groups > 1 is not implemented (group search takes "
                                      "exclude_items / allowed_items)")
        if biased:
            raise NotImplementedError("generate(item_mask=) with item_bias is not implemented (the biased search takes "
                                      "exclude_items / allowed_items)")
        if filtered:
            raise ValueError("generate: item_mask does not go with exclude_items / allowed_items: fold those into the mask")
        if candidates is None:
            raise ValueError("generate: item_mask has one column per entry of `candidates` (the sequences the Trie was built from): pass it")
        if self._closure_trie(fn) is None:
            raise ValueError("generate: item_mask needs the Trie closure form of prefix_allowed_tokens_fn "
                             "(an arbitrary callback receives batch_id and can filter per user itself)")
        n = len(candidates)
        if not isinstance(item_mask, torch.Tensor) or item_mask.dtype.is_floating_point or item_mask.dtype.is_complex or \
                tuple(item_mask.shape) != (B, n) or n < 1:
            got = (tuple(item_mask.shape), item_mask.dtype) if isinstance(item_mask, torch.Tensor) else type(item_mask).__name__
            raise ValueError(f"generate: item_mask must be a bool, uint8 or integer tensor of shape ({B}, {n}) = (B, len(candidates)), "
                             f"got {got}")
        return item_mask.detach()

    @staticmethod
    def _user_item_mask(item_mask: torch.Tensor, flat: FlatTrie, candidates, device) -> torch.Tensor:
        """``generate``'s item_mask as the contiguous uint8 (B, len(candidates)) tensor torch.ops.gram.generate_mask takes, on
        ``device``.  The preparation kernel looks a leaf up under the ONE candidate ``FlatTrie.leaf_items`` names for it, so where
        the list holds several spellings of a sequence (fewer leaves than entries) their columns are folded onto that candidate
        first.  A user whose row keeps nothing is a ``ValueError`` (one small read-back, as the lists' emptiness check)."""
        keep = item_mask.to(device).ne(0)
        B, n = keep.shape
        rank = flat.item_ranks_on(device, candidates)[1].to(torch.int64)  # (a candidate that is no leaf of the Trie: ValueError)
        if int(flat.leaf_ranges()[1][0]) < n:
            named = flat.leaf_items_on(device, candidates).to(torch.int64)[rank]  # the candidate that names each candidate's leaf
            keep = torch.zeros(B, n, dtype=torch.int32, device=device).index_add_(1, named, keep.to(torch.int32)).ne(0)
        empty = ~keep.any(dim=1)
        any_empty, first_empty = torch.stack([empty.any().long(), empty.long().argmax()]).tolist()
        if any_empty:
            raise ValueError(f"generate: item_mask leaves user {first_empty} without any item")
        return keep.to(torch.uint8).contiguous()

    def _sample_args(self, B: int, max_length: int, num_beams, num_return_sequences, temperature, top_k, top_p, uniforms, fn):
        """The arguments of ``generate(do_sample=True)`` as (R, temperature, top_k, top_p), or the refusal: everything is checked on
        the host, before the model is packed or a tensor is moved."""
        if int(num_beams) != 1:
            raise NotImplementedError("generate(do_sample=True) with num_beams > 1 (HF's beam-sample) is not implemented: "
                                      "sampling runs with num_beams=1 and num_return_sequences draws per user")
        if self._closure_trie(fn) is None:
            raise NotImplementedError("generate(do_sample=True) needs the Trie closure form of prefix_allowed_tokens_fn")
        R = 1 if num_return_sequences is None else int(num_return_sequences)
        if not 1 <= R <= _lib.GRAM_MAX_BEAMS:
            raise ValueError(f"generate(do_sample=True): num_return_sequences must lie in [1, {_lib.GRAM_MAX_BEAMS}] (got {R})")
        tau, p_top = float(temperature), float(top_p)
        k_top = 50 if top_k is None else int(top_k)  # (HF's default)
        if not (tau > 0 and tau < float("inf")):
            raise ValueError(f"generate(do_sample=True): temperature must be a positive number (got {temperature!r})")
        if not 0 < p_top <= 1:
            raise ValueError(f"generate(do_sample=True): top_p must lie in (0, 1] (got {top_p!r})")
        if k_top < 0:
            raise ValueError(f"generate(do_sample=True): top_k must be >= 0, 0 switches it off (got {top_k!r})")
        if uniforms is not None:
            want = (B, R, max_length - 1)
            if not isinstance(uniforms, torch.Tensor) or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != want:
                got = (tuple(uniforms.shape), uniforms.dtype) if isinstance(uniforms, torch.Tensor) else type(uniforms).__name__
                raise ValueError(f"generate(do_sample=True): uniforms must be a float32 tensor of shape {want} = (B, "
                                 f"num_return_sequences, max_length - 1), got {got}")
        return R, tau, k_top, p_top

    @staticmethod
    def _distinct_args(B: int, top_k, top_p, uniforms, seed, user_keys, generator):
        """What ``generate(do_sample=True, replacement=False)`` asks beyond ``_sample_args``, as (seed in [-2^63, 2^63), user_keys int64
        (B,) on the CPU), or the refusal: everything is checked on the host."""
        what = "generate(do_sample=True, replacement=False)"
        if uniforms is not None:
            raise ValueError(f"{what} takes no uniforms: its randomness is counter-based, pass seed= (and user_keys=)")
        if top_k not in (None, 0, 50) or float(top_p) != 1.0:
            raise NotImplementedError(f"{what}: top_k / top_p truncation together with exact sampling without replacement is not "
                                      f"defined here (got top_k={top_k!r}, top_p={top_p!r}); leave them at their defaults")
        if seed is None:
            seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device="cpu",
                                     generator=generator if generator is not None and generator.device.type == "cpu" else None))
        elif isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"{what}: seed must be an int (got {seed!r})")
        seed = (int(seed) + 2 ** 63) % 2 ** 64 - 2 ** 63  # (the 64-bit Philox key, as a signed word)
        if user_keys is None:
            user_keys = torch.arange(B, dtype=torch.int64)
        elif (not isinstance(user_keys, torch.Tensor) or user_keys.dtype != torch.int64 or tuple(user_keys.shape) != (B,)):
            got = (tuple(user_keys.shape), user_keys.dtype) if isinstance(user_keys, torch.Tensor) else type(user_keys).__name__
            raise ValueError(f"{what}: user_keys must be an int64 tensor of shape ({B},) = (B,), got {got}")
        return seed, user_keys.detach()

    @staticmethod
    def _user_item_lists(lists, allow: bool, B: int, flat: FlatTrie, candidates, device="cpu") -> torch.Tensor:
        """The per-user lists of ``generate`` as the int32 (B, M) tensor torch.ops.gram.generate_items takes, on ``device``: every
        row's entries first (in their order), -1 behind them, M = the longest row (at least 1).  Everything a list can get wrong is
        a ``ValueError`` here, before the search is launched.  The checks are tensor operations on ``device`` (a call's lists can
        be B x 4096 indices) with one read-back of their four results."""
        what = "allowed_items" if allow else "exclude_items"
        limit = _lib.GRAM_MAX_USER_ITEMS
        if isinstance(lists, torch.Tensor):
            if lists.dim() != 2 or lists.shape[0] != B or lists.dtype.is_floating_point or lists.dtype == torch.bool:
                raise ValueError(f"generate: {what} must be a (B, M) integer tensor padded with -1, or B lists")
            t = lists.detach().to(device, torch.int64)
        else:
            rows = [list(map(int, r)) for r in lists]
            if len(rows) != B:
                raise ValueError(f"generate: {what} needs one list per user ({B}), got {len(rows)}")
            t = torch.full((B, max(1, max(map(len, rows)))), -1, dtype=torch.int64)
            for b, r in enumerate(rows):
                t[b, : len(r)] = torch.tensor(r, dtype=torch.int64)
            t = t.to(device)
        if t.shape[1] == 0:
            t = torch.full((B, 1), -1, dtype=torch.int64, device=device)
        n = len(candidates)
        if n < 1:
            raise ValueError(f"generate: {what} indexes an empty `candidates`")
        valid = t != -1
        outside = (t < -1) | (t >= n)
        per_user = valid.sum(dim=1)
        # entries first, padding behind them
        t = torch.gather(t, 1, torch.sort((~valid).to(torch.uint8), dim=1, stable=True).indices)
        # a user must keep at least one item: count the DISTINCT leaves its list names (duplicate sequences share one)
        if torch.device(device).type == "cpu":
            rank = torch.from_numpy(flat.item_ranks(candidates))
        else:
            rank = flat.item_ranks_on(device, candidates)[1]
        r = torch.where((t >= 0) & (t < n), rank.to(torch.int64)[t.clamp(0, n - 1)], torch.full_like(t, -1)).sort(dim=1).values
        distinct = (r[:, :1] >= 0).sum(dim=1) + ((r[:, 1:] != r[:, :-1]) & (r[:, 1:] >= 0)).sum(dim=1)
        empty = distinct == 0 if allow else distinct >= int(flat.leaf_ranges()[1][0])
        any_outside, longest, any_empty, first_empty = torch.stack(
            [outside.any().long(), per_user.max(), empty.any().long(), empty.long().argmax()]).tolist()
        if any_outside:
            raise ValueError(f"generate: {what} holds an index outside [0, {n}) (-1 is the padding value)")
        if longest > limit:
            raise ValueError(f"generate: {what} has {longest} entries for one user, at most {limit} are supported")
        if any_empty:
            raise ValueError(f"generate: {what} leaves user {first_empty} without any item")
        return t[:, : max(1, longest)].to(torch.int32).contiguous()

    @torch.no_grad()
    def sequence_items(self, sequences, prefix_allowed_tokens_fn, candidates):
        """Which candidate each row of ``generate(...)["sequences"]`` spells: int32 (rows,) indices into ``candidates`` -- the
        token-id sequences the closure's Trie was built from, in the caller's order -- or -1 for a row that is not a candidate
        (HF's -inf filler beams).  Every hypothesis of a Trie-constrained search is a leaf of the Trie, so the runner needs one
        ``batch_decode`` of the candidate list per evaluation instead of one of B*K generated rows per batch
        (single_runner_gram.py:657-662); ``gram_trie_item_index`` walks the flat Trie on the device."""
        flat = self._flat_trie(prefix_allowed_tokens_fn)
        dev = self._device()
        ctrie, _keep = flat.to_device(dev)
        node_item = flat.node_items_on(dev, candidates)
        seqs = sequences.to(dev, torch.int64).contiguous()
        out = torch.empty(seqs.shape[0], dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gram_trie_item_index(C.byref(ctrie), node_item.data_ptr(), seqs.data_ptr(), seqs.shape[0], seqs.shape[1],
                                                        out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gram_trie_item_index")
        return out

    def _generate_with_callback(self, ids, mask, B, N, Lp, K, nret, max_length, length_penalty, fn, return_dict):
        """Slow path for an ARBITRARY ``prefix_allowed_tokens_fn(batch_id, sent) -> List[int]`` (HF's
        PrefixConstrainedLogitsProcessor contract): semantics preserved, one host round trip per step like the
        reference (generation_trie.py:89-95).  The model still runs on the device through the same C-ABI entry
        points (encode, decode step, LSE, beam step, finalize); only the allowed-token lists come from Python,
        uploaded each step as a one-level CSR in which row r owns node r + 1."""
        lib = _lib.load()
        dev = self._device()
        handle = self._pack()
        ws = self._get_workspace(handle, B, N, Lp, K, max_length)
        stream = torch.cuda.current_stream(dev).cuda_stream
        R, V = B * K, self.config.vocab_size
        i32 = dict(dtype=torch.int32, device=dev)
        t = dict(tokens=torch.zeros(R, **i32), node=torch.zeros(R, **i32), beam_scores=torch.zeros(R, dtype=torch.float32, device=dev),
                 seq=torch.zeros(R, max_length, **i32), anc=torch.zeros(max_length, R, **i32), done=torch.zeros(B, **i32),
                 n_hyps=torch.zeros(B, **i32), hyp_score=torch.zeros(B, K + 1, dtype=torch.float64, device=dev),
                 worst=torch.zeros(B, dtype=torch.float64, device=dev), hyp_len=torch.zeros(B, K + 1, **i32),
                 hyp_tok=torch.zeros(B, K + 1, max_length, **i32), error=torch.zeros(4, **i32))
        st = _lib.BeamState(B=B, K=K, Tmax=max_length, length_penalty=length_penalty, eos=1, pad=0,
                            **{k: v.data_ptr() for k, v in t.items()})
        logits = torch.empty(R, V, dtype=torch.float32, device=dev)
        lse = torch.empty(R, dtype=torch.float32, device=dev)

        def csr(lists):
            off = [0, 0]
            toks = []
            for l in lists:
                toks += sorted(set(int(x) for x in l))
                off.append(len(toks))
            fan = max((off[i + 1] - off[i] for i in range(1, len(off) - 1)), default=0)
            if fan > V:  # (a set of token ids: only ids outside the vocabulary can get here)
                raise _lib.GramHipError("prefix_allowed_tokens_fn returned more tokens than the vocabulary holds")
            a = torch.tensor(off, **i32)
            b = torch.tensor(toks or [0], **i32)
            c = torch.full((max(len(toks), 1),), -1, **i32)
            return _lib.Trie(a.data_ptr(), b.data_ptr(), c.data_ptr(), len(off) - 1, len(toks), max(fan, 1)), (a, b, c)

        with torch.cuda.device(dev):
            _lib.check(lib.gram_encode_fused(handle, ids.data_ptr(), mask.data_ptr(), B, N, Lp, ws.data_ptr(), ws.numel(), K,
                                             max_length, None, stream), "gram_encode_fused")
            start_trie, keep = csr([[0]])  # root -> start token, so that gram_beam_init finds node 1 for every row
            start_trie.n_nodes = 2
            _lib.check(lib.gram_beam_init(C.byref(st), C.byref(start_trie), 0, stream), "gram_beam_init")
            for step in range(max_length - 1):
                sent = t["seq"][:, : step + 1].cpu()
                lists = [fn(r // K, sent[r]) for r in range(R)]  # the reference's per-beam callback
                step_trie, keep = csr(lists)
                t["node"].copy_(torch.arange(1, R + 1, **i32))
                _lib.check(lib.gram_decode_step(handle, t["tokens"].data_ptr(), t["anc"].data_ptr(), mask.data_ptr(), B, N, Lp, K,
                                                max_length, step, ws.data_ptr(), ws.numel(), logits.data_ptr(), stream),
                           "gram_decode_step")
                _lib.check(lib.gram_row_lse(logits.data_ptr(), lse.data_ptr(), R, V, stream), "gram_row_lse")
                _lib.check(lib.gram_beam_step(C.byref(st), C.byref(step_trie), logits.data_ptr(), lse.data_ptr(), V, step + 1, K,
                                              stream), "gram_beam_step")
                torch.cuda.current_stream(dev).synchronize()  # the CSR tensors must outlive the launch
            seqs = torch.empty(B * nret, max_length, dtype=torch.int64, device=dev)
            scores = torch.empty(B * nret, dtype=torch.float32, device=dev)
            width = torch.zeros(4, **i32)
            _lib.check(lib.gram_beam_finalize(C.byref(st), nret, max_length, seqs.data_ptr(), scores.data_ptr(), width.data_ptr(),
                                              stream), "gram_beam_finalize")
            torch.cuda.current_stream(dev).synchronize()
        if int(t["error"][0]) != 0:
            _lib.check(_lib.E_BEAM, "beam search")
        seqs = seqs[:, : int(width[0])]
        return GenerateOutput(sequences=seqs, sequences_scores=scores) if return_dict else seqs

    def __del__(self):
        try:
            if self._packed is not None:
                _lib.load().gram_model_destroy(self._packed[2])
        except Exception:
            pass
