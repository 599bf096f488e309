"""PyTorch-ROCm custom ops of the scoring path, namespace ``gram``.

Thin ``torch.library`` wrappers over the C ABI (include/gram_hip.h): tensors in, tensors out, stream-ordered on
PyTorch's current HIP stream, with meta ("fake") implementations so the ops trace under ``torch.compile`` /
``FakeTensorMode``.  They are registered for the ``cuda`` device type ONLY: calling one on CPU tensors raises
(there is no CPU path in gram_amd; the CPU restatement lives in oracle/ and is test infrastructure).

    torch.ops.gram.generate          GRAM.generate's whole path (gram_generate_ex) -- what ``GRAM.generate`` calls
    torch.ops.gram.generate_items    the same path with per-user item filters (gram_user_items_prepare + gram_generate_items) --
                                     ``GRAM.generate(exclude_items= / allowed_items=)``
    torch.ops.gram.generate_mask     the same path with per-user item masks of any size (gram_user_mask_prepare + gram_generate_mask) --
                                     ``GRAM.generate(item_mask=)``
    torch.ops.gram.generate_groups   group (diverse) beam search, with or without the per-user item filters (gram_generate_groups) --
                                     ``GRAM.generate(num_beam_groups=, diversity_penalty=)``
    torch.ops.gram.item_bias_table   the potentials of per-item score biases over the Trie (gram_item_bias_table)
    torch.ops.gram.generate_bias     beam search with those potentials in every step, with or without the per-user item filters
                                     (gram_generate_bias) -- ``GRAM.generate(item_bias=)``
    torch.ops.gram.sample            Trie-constrained sampling, R draws per user with their log-probabilities (gram_sample) --
                                     ``GRAM.generate(do_sample=True)``
    torch.ops.gram.sample_items      the same with per-user item filters (gram_user_items_prepare + gram_sample_items)
    torch.ops.gram.sample_distinct   sampling WITHOUT replacement, R distinct items per user (stochastic beam search, gram_generate_sbs)
                                     -- ``GRAM.generate(do_sample=True, replacement=False)``
    torch.ops.gram.sample_distinct_items  the same with per-user item filters (gram_user_items_prepare + gram_generate_sbs_items)
    torch.ops.gram.teacher_forced    the teacher-forced decoder pass (gram_teacher_forced) -- ``GRAM.forward(labels=...)`` and
                                     ``GRAM.score_sequences``
    torch.ops.gram.teacher_forced_attn  the same pass with its cross-attention probabilities (gram_teacher_forced_ex) --
                                     ``GRAM.cross_attentions`` and ``GRAM.passage_attention``
    torch.ops.gram.teacher_forced_scores  the same pass with the probabilities summed over heads inside the kernel
                                     (gram_teacher_forced_scores): up to 16 384 fused keys, no per-head buffer --
                                     ``GRAM.passage_attention(fused=True)`` and above 4096 keys
    torch.ops.gram.score_trie        every leaf of the Trie scored in one decoder pass over its internal nodes (gram_score_trie) --
                                     ``GRAM.score_all_items``
    torch.ops.gram.linear            nn.Linear without bias: A @ W^T on the 16-bit MFMA (gram_gemm_bf16, 16-bit epilogue)
    torch.ops.gram.enc_self_attn     T5Attention self branch on (P*L, 3*inner) q|k|v rows (gram_enc_self_attn)
    torch.ops.gram.enc_self_attn_long  the same for passages of up to 512 tokens (gram_enc_self_attn_long_split)
    torch.ops.gram.cross_attn_decode the fusion read of one decoder layer and step over the beam-shared bank
    torch.ops.gram.cross_attn_long   the same over up to 16 384 fused keys (gram_cross_attn_long_split)
    torch.ops.gram.trie_step         one Trie-constrained beam-search step on dense logits (gram_row_lse + gram_beam_step)

Every op keeps its full explicit signature (``torch.library`` derives the schema from it).  What several ops do with the same
arguments is stated once, in the private helpers below the ``_check`` they are built on: ``_compaction`` / ``_trie`` build the
gram_compaction_t / gram_trie_t of a call, ``_tf_inputs`` is the validation of the three teacher-forced ops, ``_search`` the
outputs and the C call of the ``generate`` ops, ``_filter_inputs`` what the filtered ops require of the tensors they share,
``_user_items`` the validated lists of the ``*_items`` ops, ``_sample`` the
checks, outputs and C call of the two ``sample`` ops, ``_enc_self_attn`` / ``_cross_attn_inputs`` the short and long attention forms.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib

Tensor = torch.Tensor


def _stream(t: Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _ref(struct):
    """``byref`` of a ctypes struct, None (a null pointer) for None"""
    return None if struct is None else C.byref(struct)


def _check(name: str, t: Tensor, dtype, shape=None, device=None, contiguous: bool = True) -> None:
    """Everything the C ABI assumes about a tensor before its data_ptr() is taken: a wrong dtype, a transposed or sliced view or
    a shape that does not match the kernel's indexing would otherwise be silent garbage or an out-of-bounds device read."""
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous (got strides {t.stride()})")
    if t.numel() and t.data_ptr() % 16:
        raise ValueError(f"{name}: data pointer must be 16-byte aligned")
    if shape is not None:
        if t.dim() != len(shape) or any(e is not None and int(s_) != int(e) for s_, e in zip(t.shape, shape)):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple('*' if e is None else e for e in shape)}")


def _compaction(comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
                cache_x: Optional[Tensor], n_cached: int, cache_L: int) -> Optional[_lib.Compaction]:
    """The gram_compaction_t of the comp_* / cache_* arguments every whole-path op takes; None (compaction off) without a comp_map."""
    if comp_map is None:
        return None
    return _lib.Compaction(n_active=comp_map.numel(), passage_map=comp_map.data_ptr(), ids=_p(comp_ids), mask=_p(comp_mask),
                           n_cached=n_cached, cache_L=cache_L, cache_x=_p(cache_x), cache_slot=_p(cache_slot))


def _trie(child_off: Tensor, child_tok: Tensor, child_node: Tensor, max_fanout: int, min_seq_len: int) -> _lib.Trie:
    """The gram_trie_t of a Trie's three CSR arrays"""
    return _lib.Trie(child_off.data_ptr(), child_tok.data_ptr(), child_node.data_ptr(), child_off.numel() - 1, child_tok.numel(),
                     max_fanout, min_seq_len)


# ---------------------------------------------------------------------------------------------- generate
def _search(fn, what: str, input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie: _lib.Trie,
            comp: Optional[_lib.Compaction], num_beams: int, num_return_sequences: int, max_length: int, length_penalty: float,
            *extra) -> Tuple[Tensor, Tensor, Tensor]:
    """The outputs of a search, its C call ``fn`` (gram_generate_ex, or gram_generate_tail / gram_generate_items with their one
    further struct in ``extra``) and the ops' return value.  The caller has made input_ids' device the current one."""
    B, N, L = input_ids.shape
    K, nret = num_beams, num_return_sequences
    seqs = torch.empty(B * nret, max_length, dtype=torch.int64, device=input_ids.device)
    scores = torch.empty(B * nret if K > 1 else 0, dtype=torch.float32, device=input_ids.device)
    width = C.c_int32(0)
    rc = fn(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, K, nret, max_length, float(length_penalty), C.byref(trie),
            _ref(comp), *extra, workspace.data_ptr(), workspace.numel(), seqs.data_ptr(), scores.data_ptr() if K > 1 else None,
            C.byref(width), _stream(input_ids))
    _lib.check(rc, what)
    return seqs, scores, torch.tensor([width.value], dtype=torch.int32)


def _search_fake(input_ids, num_beams, num_return_sequences, max_length):
    B = input_ids.shape[0]
    return (input_ids.new_empty(B * num_return_sequences, max_length),
            input_ids.new_empty(B * num_return_sequences if num_beams > 1 else 0, dtype=torch.float32),
            torch.empty(1, dtype=torch.int32))


@torch.library.custom_op("gram::generate", mutates_args=("workspace",), device_types="cuda")
def generate(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
             trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_beams: int,
             num_return_sequences: int, max_length: int, length_penalty: float, comp_map: Optional[Tensor],
             comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor],
             n_cached: int, cache_L: int, trie_sub_rows: Optional[Tensor] = None, trie_d_tail: int = 0,
             trie_tail_steps: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """input_ids i64 (B,N,L), attention_mask u8 (B,N,L), ``handle`` a gram_model_t* as int, ``workspace`` a u8 scratch tensor of
    gram_workspace_bytes; the Trie as its CSR arrays (gram_trie_t); comp_* / cache_* the gram_compaction_t fields (None = off).
    trie_sub_rows i32 (n_nodes,) / trie_d_tail / trie_tail_steps: the Trie's tail tables (gram_trie_tail_t, ``FlatTrie.tail_tables``);
    given, the call is gram_generate_tail and ``workspace`` must hold gram_workspace_bytes_tail.  Returns (sequences i64 (B*nret, max_length), sequences_scores f32 (B*nret) -- empty for greedy search --, width i32 (1,))."""
    lib = _lib.load()
    dev = input_ids.device
    # (unlike generate_items, this op does not validate its tensors: ``GRAM.generate`` prepares them, and this is the benchmarked path)
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    fn, tail = lib.gram_generate_ex, ()
    if trie_sub_rows is not None and trie_d_tail > 0:
        _check("trie_sub_rows", trie_sub_rows, torch.int32, (trie_child_off.numel() - 1,), dev)
        fn, tail = lib.gram_generate_tail, (C.byref(_lib.TrieTail(trie_sub_rows.data_ptr(), int(trie_d_tail), int(trie_tail_steps))),)
    with torch.cuda.device(dev):
        return _search(fn, "gram_generate", input_ids, attention_mask, handle, workspace, trie, comp, num_beams, num_return_sequences,
                       max_length, length_penalty, *tail)


@generate.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout,
      trie_min_seq_len, num_beams, num_return_sequences, max_length, length_penalty, comp_map, comp_ids, comp_mask, cache_slot,
      cache_x, n_cached, cache_L, trie_sub_rows=None, trie_d_tail=0, trie_tail_steps=0):
    return _search_fake(input_ids, num_beams, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- generate with per-user item filters
def _filter_inputs(input_ids: Tensor, attention_mask: Tensor, trie_child_off: Tensor, trie_child_tok: Tensor, trie_child_node: Tensor,
                   leaf_lo: Tensor, leaf_hi: Tensor, more) -> int:
    """What every op with a per-user filter (lists or masks) requires of the tensors they share, and of the int32 tensors in
    ``more`` ((name, tensor, shape), ...): dtype, device, layout and shape.  input_ids is (B, N, L).  Returns n_nodes."""
    B, N, L = input_ids.shape
    dev = input_ids.device
    n_nodes = trie_child_off.numel() - 1
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, (B, N, L), dev)
    for name, t, shape in (("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),)), ("leaf_lo", leaf_lo, (n_nodes,)),
                           ("leaf_hi", leaf_hi, (n_nodes,)), *more):
        _check(name, t, torch.int32, shape, dev)
    return n_nodes


def _user_items(op: str, input_ids: Tensor, attention_mask: Tensor, trie_child_off: Tensor, trie_child_tok: Tensor,
                trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, comp_map, comp_ids, comp_mask, cache_slot, cache_x,
                n_cached: int, cache_L: int, leaf_lo: Tensor, leaf_hi: Tensor, item_rank: Tensor, items: Tensor, allow: bool):
    """What the two ``*_items`` ops require of their tensors, or a ``ValueError`` in ``op``'s name; then the lists as sorted distinct
    leaf ranks on the device (gram_user_items_prepare, on input_ids' current stream).  Returns (gram_trie_t, gram_compaction_t or
    None, gram_user_items_t, the tensors the last one points into)."""
    lib = _lib.load()
    if input_ids.dim() != 3 or items.dim() != 2:
        raise ValueError(f"{op}: input_ids must be (B, N, L) and items (B, M)")
    B, N, L = input_ids.shape
    dev = input_ids.device
    M = items.shape[1]
    n_nodes = _filter_inputs(input_ids, attention_mask, trie_child_off, trie_child_tok, trie_child_node, leaf_lo, leaf_hi,
                             (("item_rank", item_rank, (None,)), ("items", items, (B, None))))
    if n_nodes < 1 or item_rank.numel() < 1 or not 1 <= M <= _lib.GRAM_MAX_USER_ITEMS:
        raise ValueError(f"{op}: need a Trie, at least one candidate and 1 <= M <= {_lib.GRAM_MAX_USER_ITEMS} (got M={M})")
    # candidate indices index item_rank on the device: out-of-range ones are refused here, not read there
    lo_i, hi_i = torch.stack([items.min(), items.max()]).tolist()
    if lo_i < -1 or hi_i >= item_rank.numel():
        raise ValueError(f"{op}: items must lie in [0, {item_rank.numel()}) or be the padding value -1")
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    ranks = torch.empty(B, M, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    ui = _lib.UserItems(leaf_lo.data_ptr(), leaf_hi.data_ptr(), ranks.data_ptr(), count.data_ptr(), M,
                        _lib.ITEMS_ALLOW if allow else _lib.ITEMS_EXCLUDE)
    with torch.cuda.device(dev):
        _lib.check(lib.gram_user_items_prepare(item_rank.data_ptr(), item_rank.numel(), items.data_ptr(), B, M, ranks.data_ptr(),
                                               count.data_ptr(), M, _stream(input_ids)), "gram_user_items_prepare")
    return trie, comp, ui, (ranks, count)


def _optional_user_items(op: str, input_ids: Tensor, attention_mask: Tensor, trie_child_off: Tensor, trie_child_tok: Tensor,
                         trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, comp_map, comp_ids, comp_mask, cache_slot,
                         cache_x, n_cached: int, cache_L: int, leaf_lo, leaf_hi, item_rank, items, allow: bool):
    """The optional lists of ``generate_groups`` and ``generate_bias``: the four list tensors come together -- then ``_user_items`` --
    or not at all -- then the plain inputs are validated here.  Returns (gram_trie_t, gram_compaction_t or None, the argument for
    the call's ``items`` -- a reference to the gram_user_items_t or None --, what it points into: keep it until the call returns)."""
    lists = (leaf_lo, leaf_hi, item_rank, items)
    if any(t is not None for t in lists):
        if any(t is None for t in lists):
            raise ValueError(f"{op}: leaf_lo, leaf_hi, item_rank and items come together")
        trie, comp, ui, keep = _user_items(op, input_ids, attention_mask, trie_child_off, trie_child_tok, trie_child_node,
                                           trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
                                           cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
        return trie, comp, C.byref(ui), (ui, keep)
    if input_ids.dim() != 3:
        raise ValueError(f"{op}: input_ids must be (B, N, L)")
    dev = input_ids.device
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, tuple(input_ids.shape), dev)
    for name, t, shape in (("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),))):
        _check(name, t, torch.int32, shape, dev)
    return (_trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len),
            _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L), None, None)


@torch.library.custom_op("gram::generate_items", mutates_args=("workspace",), device_types="cuda")
def generate_items(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                   trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_beams: int,
                   num_return_sequences: int, max_length: int, length_penalty: float, comp_map: Optional[Tensor],
                   comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor],
                   n_cached: int, cache_L: int, leaf_lo: Tensor, leaf_hi: Tensor, item_rank: Tensor, items: Tensor,
                   allow: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """``generate`` (same inputs, same outputs) with every user searching its own view of the Trie (gram_user_items_t): leaf_lo /
    leaf_hi i32 (n_nodes,) the leaf-rank range below every node, item_rank i32 (n_items,) the leaf rank of every candidate, items
    i32 (B, M) each user's candidate indices padded with -1, M <= 4096; ``allow``: the lists are what a user may get (else what it
    may not).  The lists become sorted distinct ranks on the device (gram_user_items_prepare), then gram_generate_items runs."""
    trie, comp, ui, _keep = _user_items("generate_items", input_ids, attention_mask, trie_child_off, trie_child_tok, trie_child_node,
                                        trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
                                        cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
    with torch.cuda.device(input_ids.device):
        return _search(_lib.load().gram_generate_items, "gram_generate_items", input_ids, attention_mask, handle, workspace, trie, comp,
                       num_beams, num_return_sequences, max_length, length_penalty, C.byref(ui))


@generate_items.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout,
      trie_min_seq_len, num_beams, num_return_sequences, max_length, length_penalty, comp_map, comp_ids, comp_mask, cache_slot,
      cache_x, n_cached, cache_L, leaf_lo, leaf_hi, item_rank, items, allow):
    return _search_fake(input_ids, num_beams, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- generate with per-user item masks
@torch.library.custom_op("gram::generate_mask", mutates_args=("workspace",), device_types="cuda")
def generate_mask(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                  trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_beams: int,
                  num_return_sequences: int, max_length: int, length_penalty: float, comp_map: Optional[Tensor],
                  comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor],
                  n_cached: int, cache_L: int, leaf_lo: Tensor, leaf_hi: Tensor, leaf_item: Tensor,
                  item_mask: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``generate_items`` (same inputs) with the users' sets as a mask of any size in the lists' place (gram_user_mask_t): leaf_item
    i32 (n_leaves,) the candidate that names the leaf of every leaf rank (``FlatTrie.leaf_items``), item_mask u8 (B, n_items),
    rows contiguous (any row stride), non-zero = the user may get the candidate.  The records -- B * (n_leaves / 32 + 1) * 8 bytes
    -- are allocated here, next to the workspace, and written by gram_user_mask_prepare on input_ids' current stream; then
    gram_generate_mask runs.  Returns ``generate``'s three outputs and count i32 (B,) on the device: the leaves every user keeps
    (a user with 0 has no item: the caller's to refuse)."""
    lib = _lib.load()
    if input_ids.dim() != 3 or item_mask.dim() != 2 or leaf_item.dim() != 1:
        raise ValueError("generate_mask: input_ids must be (B, N, L), item_mask (B, n_items) and leaf_item (n_leaves,)")
    B = input_ids.shape[0]
    dev = input_ids.device
    n_leaves, n_items = leaf_item.numel(), item_mask.shape[1]
    n_nodes = _filter_inputs(input_ids, attention_mask, trie_child_off, trie_child_tok, trie_child_node, leaf_lo, leaf_hi,
                             (("leaf_item", leaf_item, (n_leaves,)),))
    if item_mask.dtype != torch.uint8 or item_mask.device != dev or item_mask.shape[0] != B:
        raise ValueError(f"generate_mask: item_mask must be a uint8 tensor of shape ({B}, n_items) on {dev}")
    if n_nodes < 1 or n_leaves < 1 or n_items < 1 or item_mask.stride(1) != 1 or (B > 1 and item_mask.stride(0) < n_items):
        raise ValueError("generate_mask: need a Trie, at least one leaf and one candidate, and item_mask rows that are contiguous")
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    stride = int(lib.gram_user_mask_words(n_leaves))
    words = torch.empty(B, stride, 2, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    um = _lib.UserMask(leaf_lo.data_ptr(), leaf_hi.data_ptr(), words.data_ptr(), stride, n_leaves)
    with torch.cuda.device(dev):
        _lib.check(lib.gram_user_mask_prepare(item_mask.data_ptr(), item_mask.stride(0) if B > 1 else n_items, B, n_items,
                                              leaf_item.data_ptr(), n_leaves, words.data_ptr(), stride, count.data_ptr(),
                                              _stream(input_ids)), "gram_user_mask_prepare")
        return (*_search(lib.gram_generate_mask, "gram_generate_mask", input_ids, attention_mask, handle, workspace, trie, comp,
                         num_beams, num_return_sequences, max_length, length_penalty, C.byref(um)), count)


@generate_mask.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout,
      trie_min_seq_len, num_beams, num_return_sequences, max_length, length_penalty, comp_map, comp_ids, comp_mask, cache_slot,
      cache_x, n_cached, cache_L, leaf_lo, leaf_hi, leaf_item, item_mask):
    return (*_search_fake(input_ids, num_beams, num_return_sequences, max_length),
            input_ids.new_empty(input_ids.shape[0], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- group (diverse) beam search
def _check_groups(op: str, num_beams: int, num_beam_groups: int, diversity_penalty: float) -> None:
    """The (K, G, penalty) of a group search, or a ``ValueError`` in ``op``'s name (what gram_generate_groups answers with GRAM_E_ARG)"""
    K, G, lam = int(num_beams), int(num_beam_groups), float(diversity_penalty)
    if not 2 <= K <= _lib.GRAM_MAX_BEAMS or G < 1 or G > K or K % G:
        raise ValueError(f"{op}: need 2 <= num_beams <= {_lib.GRAM_MAX_BEAMS} and num_beam_groups a divisor of it "
                         f"(got num_beams={K}, num_beam_groups={G})")
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"{op}: diversity_penalty must be a finite number >= 0 (got {diversity_penalty!r})")


@torch.library.custom_op("gram::generate_groups", mutates_args=("workspace",), device_types="cuda")
def generate_groups(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                    trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_beams: int,
                    num_return_sequences: int, max_length: int, length_penalty: float, num_beam_groups: int, diversity_penalty: float,
                    comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
                    cache_x: Optional[Tensor], n_cached: int, cache_L: int, leaf_lo: Optional[Tensor] = None,
                    leaf_hi: Optional[Tensor] = None, item_rank: Optional[Tensor] = None, items: Optional[Tensor] = None,
                    allow: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """Group (diverse) beam search, HF ``group_beam_search`` on the Trie (gram_generate_groups): ``generate``'s inputs and outputs,
    ``workspace`` of gram_workspace_bytes, plus num_beam_groups (a divisor of num_beams >= 2) and diversity_penalty (finite, >= 0).
    The optional tail leaf_lo / leaf_hi / item_rank / items / allow is ``generate_items``'s: given (all four tensors), every user
    searches its own view of the Trie, the lists validated and prepared the same way."""
    _check_groups("generate_groups", num_beams, num_beam_groups, diversity_penalty)
    if not 1 <= num_return_sequences <= num_beams:
        raise ValueError("generate_groups: need 1 <= num_return_sequences <= num_beams")
    trie, comp, ui_ref, _keep = _optional_user_items("generate_groups", input_ids, attention_mask, trie_child_off, trie_child_tok,
                                                     trie_child_node, trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask,
                                                     cache_slot, cache_x, n_cached, cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
    with torch.cuda.device(input_ids.device):
        return _search(_lib.load().gram_generate_groups, "gram_generate_groups", input_ids, attention_mask, handle, workspace, trie, comp,
                       num_beams, num_return_sequences, max_length, length_penalty, int(num_beam_groups), float(diversity_penalty), ui_ref)


@generate_groups.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout,
      trie_min_seq_len, num_beams, num_return_sequences, max_length, length_penalty, num_beam_groups, diversity_penalty, comp_map,
      comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L, leaf_lo=None, leaf_hi=None, item_rank=None, items=None, allow=False):
    return _search_fake(input_ids, num_beams, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- per-item score biases
@torch.library.custom_op("gram::item_bias_table", mutates_args=(), device_types="cuda")
def item_bias_table(item_bias: Tensor, leaf_item: Tensor, leaf_lo: Tensor, leaf_hi: Tensor, trie_child_off: Tensor,
                    trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, start_token: int,
                    lookahead: bool) -> Tensor:
    """The potentials of a biased search (gram_item_bias_table): item_bias f32 (rows, n_items), leaf_item i32
    (n_leaves,) the candidate of every leaf rank (``FlatTrie.leaf_items``), leaf_lo / leaf_hi i32 (n_nodes,) and the Trie's CSR
    arrays.  Returns phi f32 (rows, n_nodes): a leaf's entry is its item's bias, an internal node's the largest entry below it
    (``lookahead``) or 0, the root's and the start node's 0.  Finite values are the caller's business (``GRAM.generate`` checks)."""
    dev = item_bias.device
    if item_bias.dim() != 2 or item_bias.shape[0] < 1 or item_bias.shape[1] < 1:
        raise ValueError("item_bias_table: item_bias must be (rows, n_items)")
    n_nodes = trie_child_off.numel() - 1
    _check("item_bias", item_bias, torch.float32)
    for name, t, shape in (("leaf_item", leaf_item, (None,)), ("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),)), ("leaf_lo", leaf_lo, (n_nodes,)),
                           ("leaf_hi", leaf_hi, (n_nodes,))):
        _check(name, t, torch.int32, shape, dev)
    rows, n_items = item_bias.shape
    if n_nodes < 1 or leaf_item.numel() < 1 or rows > 65535:
        raise ValueError("item_bias_table: need a Trie with at least one leaf and at most 65535 rows of biases")
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    phi = torch.empty(rows, n_nodes, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gram_item_bias_table(item_bias.data_ptr(), n_items, rows, n_items, leaf_item.data_ptr(), leaf_item.numel(),
                                                    leaf_lo.data_ptr(), leaf_hi.data_ptr(), C.byref(trie), int(start_token),
                                                    1 if lookahead else 0, phi.data_ptr(), _stream(item_bias)), "gram_item_bias_table")
    return phi


@item_bias_table.register_fake
def _(item_bias, leaf_item, leaf_lo, leaf_hi, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      start_token, lookahead):
    return item_bias.new_empty(item_bias.shape[0], trie_child_off.numel() - 1)


@torch.library.custom_op("gram::generate_bias", mutates_args=("workspace",), device_types="cuda")
def generate_bias(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                  trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_beams: int,
                  num_return_sequences: int, max_length: int, length_penalty: float, phi: Tensor, comp_map: Optional[Tensor],
                  comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor],
                  n_cached: int, cache_L: int, leaf_lo: Optional[Tensor] = None, leaf_hi: Optional[Tensor] = None,
                  item_rank: Optional[Tensor] = None, items: Optional[Tensor] = None,
                  allow: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """Beam search with per-item score biases (gram_generate_bias): ``generate``'s inputs and outputs,
    ``workspace`` of gram_workspace_bytes, plus phi f32 (1, n_nodes) -- shared by all users -- or (B, n_nodes), the potentials
    ``item_bias_table`` returns; num_beams >= 2.  The optional tail leaf_lo / leaf_hi / item_rank / items / allow is
    ``generate_items``'s: given (all four tensors), every user searches its own view of the Trie."""
    if not 2 <= num_beams <= _lib.GRAM_MAX_BEAMS or not 1 <= num_return_sequences <= num_beams:
        raise ValueError(f"generate_bias: need 2 <= num_beams <= {_lib.GRAM_MAX_BEAMS} and 1 <= num_return_sequences <= num_beams")
    if input_ids.dim() != 3:
        raise ValueError("generate_bias: input_ids must be (B, N, L)")
    dev = input_ids.device
    n_nodes = trie_child_off.numel() - 1
    if phi.dim() != 2 or phi.shape[0] not in (1, input_ids.shape[0]):
        raise ValueError(f"generate_bias: phi must be (1, n_nodes) or (B, n_nodes), got {tuple(phi.shape)}")
    _check("phi", phi, torch.float32, (None, n_nodes), dev)
    trie, comp, ui_ref, _keep = _optional_user_items("generate_bias", input_ids, attention_mask, trie_child_off, trie_child_tok,
                                                     trie_child_node, trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask,
                                                     cache_slot, cache_x, n_cached, cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
    with torch.cuda.device(dev):
        return _search(_lib.load().gram_generate_bias, "gram_generate_bias", input_ids, attention_mask, handle, workspace, trie, comp,
                       num_beams, num_return_sequences, max_length, length_penalty, phi.data_ptr(),
                       0 if phi.shape[0] == 1 else n_nodes, ui_ref)


@generate_bias.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout,
      trie_min_seq_len, num_beams, num_return_sequences, max_length, length_penalty, phi, comp_map, comp_ids, comp_mask, cache_slot,
      cache_x, n_cached, cache_L, leaf_lo=None, leaf_hi=None, item_rank=None, items=None, allow=False):
    return _search_fake(input_ids, num_beams, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- Trie-constrained sampling
def _sample(fn, what: str, input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie: _lib.Trie,
            comp: Optional[_lib.Compaction], num_return_sequences: int, max_length: int, temperature: float, top_k: int, top_p: float,
            uniforms: Tensor, *extra) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The checks, the outputs and the C call ``fn`` (gram_sample, or gram_sample_items with its lists in ``extra``) of the two
    ``sample`` ops, and their return value."""
    if input_ids.dim() != 3:
        raise ValueError(f"{what}: input_ids must be (B, N, L)")
    B, N, L = input_ids.shape
    R, dev = num_return_sequences, input_ids.device
    if not 1 <= R <= _lib.GRAM_MAX_BEAMS or not 2 <= max_length <= _lib.GRAM_MAX_DEC_LEN:
        raise ValueError(f"{what}: need 1 <= num_return_sequences <= {_lib.GRAM_MAX_BEAMS} and 2 <= max_length <= {_lib.GRAM_MAX_DEC_LEN}")
    if not temperature > 0 or top_k < 0 or not 0 < top_p <= 1:
        raise ValueError(f"{what}: need temperature > 0, top_k >= 0 and 0 < top_p <= 1")
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, (B, N, L), dev)
    _check("uniforms", uniforms, torch.float32, (B, R, max_length - 1), dev)
    prm = _lib.SampleParams(float(temperature), int(top_k), float(top_p))
    seqs = torch.empty(B * R, max_length, dtype=torch.int64, device=dev)
    model_lp = torch.empty(B * R, dtype=torch.float32, device=dev)
    sample_lp = torch.empty(B * R, dtype=torch.float32, device=dev)
    width = C.c_int32(0)
    with torch.cuda.device(dev):
        rc = fn(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, R, max_length, C.byref(trie), _ref(comp), *extra,
                C.byref(prm), uniforms.data_ptr(), workspace.data_ptr(), workspace.numel(), seqs.data_ptr(), model_lp.data_ptr(),
                sample_lp.data_ptr(), C.byref(width), _stream(input_ids))
    _lib.check(rc, what)
    return seqs, model_lp, sample_lp, torch.tensor([width.value], dtype=torch.int32)


def _sample_fake(input_ids, num_return_sequences, max_length):
    rows = input_ids.shape[0] * num_return_sequences
    f = dict(dtype=torch.float32)
    return (input_ids.new_empty(rows, max_length), input_ids.new_empty(rows, **f), input_ids.new_empty(rows, **f),
            torch.empty(1, dtype=torch.int32))


@torch.library.custom_op("gram::sample", mutates_args=("workspace",), device_types="cuda")
def sample(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor, trie_child_tok: Tensor,
           trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, num_return_sequences: int, max_length: int,
           temperature: float, top_k: int, top_p: float, uniforms: Tensor, comp_map: Optional[Tensor], comp_ids: Optional[Tensor],
           comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor], n_cached: int,
           cache_L: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """HF ``sample`` on the Trie (gram_sample): R = num_return_sequences draws per user.  input_ids / attention_mask / handle / the Trie /
    comp_* / cache_* as ``generate``; ``workspace`` a u8 scratch tensor of gram_workspace_bytes_sample; temperature > 0, top_k >= 0 (0 =
    off), 0 < top_p <= 1; uniforms f32 (B, R, max_length - 1) in [0, 1): row (b, r) consumes uniforms[b, r, t] at step t (inverse-CDF
    sampling).  Returns (sequences i64 (B*R, max_length) user-major, the model's log-probability of each row f32 (B*R), its
    log-probability under the warped distribution it was drawn from f32 (B*R), width i32 (1,))."""
    for name, t, shape in (("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),))):
        _check(name, t, torch.int32, shape, input_ids.device)
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    return _sample(_lib.load().gram_sample, "gram_sample", input_ids, attention_mask, handle, workspace, trie, comp, num_return_sequences,
                   max_length, temperature, top_k, top_p, uniforms)


@sample.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      num_return_sequences, max_length, temperature, top_k, top_p, uniforms, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
      cache_L):
    return _sample_fake(input_ids, num_return_sequences, max_length)


@torch.library.custom_op("gram::sample_items", mutates_args=("workspace",), device_types="cuda")
def sample_items(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                 trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int,
                 num_return_sequences: int, max_length: int, temperature: float, top_k: int, top_p: float, uniforms: Tensor,
                 comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
                 cache_x: Optional[Tensor], n_cached: int, cache_L: int, leaf_lo: Tensor, leaf_hi: Tensor, item_rank: Tensor,
                 items: Tensor, allow: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``sample`` (same inputs, same outputs) with every user drawing from its own view of the Trie: the lists of ``generate_items``
    (leaf_lo / leaf_hi / item_rank / items / allow), prepared the same way, then gram_sample_items."""
    trie, comp, ui, _keep = _user_items("sample_items", input_ids, attention_mask, trie_child_off, trie_child_tok, trie_child_node,
                                        trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
                                        cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
    return _sample(_lib.load().gram_sample_items, "gram_sample_items", input_ids, attention_mask, handle, workspace, trie, comp,
                   num_return_sequences, max_length, temperature, top_k, top_p, uniforms, C.byref(ui))


@sample_items.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      num_return_sequences, max_length, temperature, top_k, top_p, uniforms, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
      cache_L, leaf_lo, leaf_hi, item_rank, items, allow):
    return _sample_fake(input_ids, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- sampling without replacement
def _sample_distinct(fn, what: str, input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie: _lib.Trie,
                     comp: Optional[_lib.Compaction], num_return_sequences: int, max_length: int, temperature: float, seed: int,
                     user_keys: Tensor, *extra) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The checks, the outputs and the C call ``fn`` (gram_generate_sbs, or gram_generate_sbs_items with its lists in ``extra``) of
    the two ``sample_distinct`` ops, and their return value."""
    if input_ids.dim() != 3:
        raise ValueError(f"{what}: input_ids must be (B, N, L)")
    B, N, L = input_ids.shape
    R, dev = num_return_sequences, input_ids.device
    if not 1 <= R <= _lib.GRAM_MAX_BEAMS or not 2 <= max_length <= _lib.GRAM_MAX_DEC_LEN:
        raise ValueError(f"{what}: need 1 <= num_return_sequences <= {_lib.GRAM_MAX_BEAMS} and 2 <= max_length <= {_lib.GRAM_MAX_DEC_LEN}")
    if not 0 < temperature < float("inf"):
        raise ValueError(f"{what}: need a finite temperature > 0")
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, (B, N, L), dev)
    _check("user_keys", user_keys, torch.int64, (B,), dev)
    seqs = torch.empty(B * R, max_length, dtype=torch.int64, device=dev)
    model_lp, sample_lp, perturbed = (torch.empty(B * R, dtype=torch.float32, device=dev) for _ in range(3))
    width = C.c_int32(0)
    with torch.cuda.device(dev):
        rc = fn(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, R, max_length, C.byref(trie), _ref(comp), *extra,
                float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF, user_keys.data_ptr(), workspace.data_ptr(), workspace.numel(),
                seqs.data_ptr(), model_lp.data_ptr(), sample_lp.data_ptr(), perturbed.data_ptr(), C.byref(width), _stream(input_ids))
    _lib.check(rc, what)
    return seqs, model_lp, sample_lp, perturbed, torch.tensor([width.value], dtype=torch.int32)


def _sample_distinct_fake(input_ids, num_return_sequences, max_length):
    rows = input_ids.shape[0] * num_return_sequences
    f = dict(dtype=torch.float32)
    return (input_ids.new_empty(rows, max_length), input_ids.new_empty(rows, **f), input_ids.new_empty(rows, **f),
            input_ids.new_empty(rows, **f), torch.empty(1, dtype=torch.int32))


@torch.library.custom_op("gram::sample_distinct", mutates_args=("workspace",), device_types="cuda")
def sample_distinct(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                    trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int,
                    num_return_sequences: int, max_length: int, temperature: float, seed: int, user_keys: Tensor,
                    comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
                    cache_x: Optional[Tensor], n_cached: int, cache_L: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Sampling without replacement on the Trie, stochastic beam search (gram_generate_sbs): R = num_return_sequences DISTINCT items per
    user in Plackett-Luce order.  input_ids / attention_mask / handle / the Trie / comp_* / cache_* as ``generate``; ``workspace`` a u8
    scratch tensor of gram_workspace_bytes_sbs; temperature > 0; ``seed`` the 64-bit Philox key (taken modulo 2^64); user_keys i64 (B,):
    a user's draw depends on (seed, its key, the model's logits) only.  Returns (sequences i64 (B*R, max_length) user-major in
    descending order of the perturbed score, the model's log-probability of each row f32 (B*R), its log-probability under the
    Trie-renormalised distribution f32 (B*R), its perturbed score f32 (B*R), width i32 (1,)); a user with fewer than R items gets rows
    of the start token and padding with -inf in all three."""
    for name, t, shape in (("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),))):
        _check(name, t, torch.int32, shape, input_ids.device)
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    return _sample_distinct(_lib.load().gram_generate_sbs, "gram_generate_sbs", input_ids, attention_mask, handle, workspace, trie, comp,
                            num_return_sequences, max_length, temperature, seed, user_keys)


@sample_distinct.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      num_return_sequences, max_length, temperature, seed, user_keys, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
      cache_L):
    return _sample_distinct_fake(input_ids, num_return_sequences, max_length)


@torch.library.custom_op("gram::sample_distinct_items", mutates_args=("workspace",), device_types="cuda")
def sample_distinct_items(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor,
                          trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int,
                          num_return_sequences: int, max_length: int, temperature: float, seed: int, user_keys: Tensor,
                          comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor],
                          cache_slot: Optional[Tensor], cache_x: Optional[Tensor], n_cached: int, cache_L: int, leaf_lo: Tensor,
                          leaf_hi: Tensor, item_rank: Tensor, items: Tensor,
                          allow: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``sample_distinct`` (same inputs, same outputs) with every user drawing from its own view of the Trie: the lists of
    ``generate_items`` (leaf_lo / leaf_hi / item_rank / items / allow), prepared the same way, then gram_generate_sbs_items."""
    trie, comp, ui, _keep = _user_items("sample_distinct_items", input_ids, attention_mask, trie_child_off, trie_child_tok,
                                        trie_child_node, trie_max_fanout, trie_min_seq_len, comp_map, comp_ids, comp_mask, cache_slot,
                                        cache_x, n_cached, cache_L, leaf_lo, leaf_hi, item_rank, items, allow)
    return _sample_distinct(_lib.load().gram_generate_sbs_items, "gram_generate_sbs_items", input_ids, attention_mask, handle, workspace,
                            trie, comp, num_return_sequences, max_length, temperature, seed, user_keys, C.byref(ui))


@sample_distinct_items.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      num_return_sequences, max_length, temperature, seed, user_keys, comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached,
      cache_L, leaf_lo, leaf_hi, item_rank, items, allow):
    return _sample_distinct_fake(input_ids, num_return_sequences, max_length)


# ---------------------------------------------------------------------------------------------- teacher-forced pass
def _tf_inputs(op: str, input_ids: Tensor, attention_mask: Tensor, decoder_input_ids: Tensor, labels: Tensor,
               vocab_size: int) -> Tuple[int, int, int, int, int]:
    """What the three teacher-forced ops require of input_ids i64 (B,N,L), attention_mask u8 (B,N,L), decoder_input_ids i32 (B,C,T)
    in [0, vocab_size) and labels i32 (B,C,T) < vocab_size (< 0 = ignored), or a ``ValueError`` in ``op``'s name; returns
    (B, N, L, C, T).  The range check is the call's one read-back from the device."""
    dev = input_ids.device
    if input_ids.dim() != 3 or decoder_input_ids.dim() != 3:
        raise ValueError(f"{op}: input_ids must be (B, N, L) and decoder_input_ids (B, C, T)")
    B, N, L = input_ids.shape
    _, Cn, T = decoder_input_ids.shape
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, (B, N, L), dev)
    _check("decoder_input_ids", decoder_input_ids, torch.int32, (B, None, None), dev)
    _check("labels", labels, torch.int32, (B, Cn, T), dev)
    if not 1 <= T <= _lib.GRAM_MAX_DEC_LEN or Cn < 1:
        raise ValueError(f"{op}: need 1 <= T <= {_lib.GRAM_MAX_DEC_LEN} and C >= 1 (got C={Cn}, T={T})")
    # token ids index the embedding and lm_head tables on the device: out-of-range ones are refused here, not read there
    lo_d, hi_d, hi_l = torch.stack([decoder_input_ids.min(), decoder_input_ids.max(), labels.max()]).tolist()
    if lo_d < 0 or hi_d >= vocab_size or hi_l >= vocab_size:
        raise ValueError(f"{op}: decoder_input_ids must lie in [0, {vocab_size}) and labels below {vocab_size}")
    return B, N, L, Cn, T


@torch.library.custom_op("gram::teacher_forced", mutates_args=("workspace",), device_types="cuda")
def teacher_forced(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, decoder_input_ids: Tensor, labels: Tensor,
                   vocab_size: int, want_logits: bool, comp_map: Optional[Tensor], comp_ids: Optional[Tensor],
                   comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor], n_cached: int,
                   cache_L: int) -> Tuple[Tensor, Tensor, Tensor]:
    """input_ids i64 (B,N,L), attention_mask u8 (B,N,L), ``handle`` a gram_model_t* as int, ``workspace`` a u8 scratch tensor of
    gram_workspace_bytes_tf; decoder_input_ids i32 (B,C,T) in [0, vocab_size), labels i32 (B,C,T) < vocab_size (< 0 = ignored);
    comp_* / cache_* the gram_compaction_t fields (None = off).  Returns (logits f32 (B,C,T,V) -- empty unless want_logits --,
    token log-probs f32 (B,C,T) -- 0 where the label is ignored --, their per-sequence sums f32 (B,C))."""
    lib = _lib.load()
    B, N, L, Cn, T = _tf_inputs("teacher_forced", input_ids, attention_mask, decoder_input_ids, labels, vocab_size)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    f = dict(dtype=torch.float32, device=input_ids.device)
    logits = torch.empty((B, Cn, T, vocab_size) if want_logits else (0,), **f)
    tok = torch.empty(B, Cn, T, **f)
    seq = torch.empty(B, Cn, **f)
    with torch.cuda.device(input_ids.device):
        rc = lib.gram_teacher_forced(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, _ref(comp),
                                     decoder_input_ids.data_ptr(), labels.data_ptr(), Cn, T, workspace.data_ptr(), workspace.numel(),
                                     logits.data_ptr() if want_logits else None, tok.data_ptr(), seq.data_ptr(), _stream(input_ids))
    _lib.check(rc, "gram_teacher_forced")
    return logits, tok, seq


@teacher_forced.register_fake
def _(input_ids, attention_mask, handle, workspace, decoder_input_ids, labels, vocab_size, want_logits, comp_map, comp_ids, comp_mask,
      cache_slot, cache_x, n_cached, cache_L):
    B, Cn, T = decoder_input_ids.shape
    f = dict(dtype=torch.float32)
    return (decoder_input_ids.new_empty((B, Cn, T, vocab_size) if want_logits else (0,), **f),
            decoder_input_ids.new_empty(B, Cn, T, **f), decoder_input_ids.new_empty(B, Cn, **f))


@torch.library.custom_op("gram::teacher_forced_attn", mutates_args=("workspace",), device_types="cuda")
def teacher_forced_attn(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, decoder_input_ids: Tensor,
                        labels: Tensor, vocab_size: int, n_dec_layers: int, n_heads: int, want_probs: bool, want_scores: bool,
                        comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
                        cache_x: Optional[Tensor], n_cached: int, cache_L: int) -> Tuple[Tensor, Tensor, Tensor]:
    """The teacher-forced pass of ``teacher_forced`` (same inputs, validated by the same ``_tf_inputs``) with its cross-attention
    probabilities (gram_teacher_forced_ex).  ``n_dec_layers`` / ``n_heads`` are the model's (they size the outputs).  Returns
    (probs f32 (n_dec_layers, B, H, C*T, N*L) -- empty unless want_probs: then one layer at a time lives in a scratch tensor --,
    token_scores f32 (B, C*T, N*L) = their sum over layers and heads, passage_scores f32 (B, C*T, N) = per passage the sum over its
    valid keys / (valid keys * n_dec_layers * n_heads), NaN for a passage without one -- both empty unless want_scores)."""
    lib = _lib.load()
    if not (want_probs or want_scores):
        raise ValueError("teacher_forced_attn: nothing requested (want_probs / want_scores)")
    if n_dec_layers < 1 or n_heads < 1:
        raise ValueError("teacher_forced_attn: need n_dec_layers >= 1, n_heads >= 1")
    B, N, L, Cn, T = _tf_inputs("teacher_forced_attn", input_ids, attention_mask, decoder_input_ids, labels, vocab_size)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    Q, S = Cn * T, N * L
    f = dict(dtype=torch.float32, device=input_ids.device)
    probs = torch.empty((n_dec_layers, B, n_heads, Q, S) if want_probs else (0,), **f)
    layer = None if want_probs else torch.empty(B, n_heads, Q, S, **f)
    tsc = torch.empty((B, Q, S) if want_scores else (0,), **f)
    psc = torch.empty((B, Q, N) if want_scores else (0,), **f)
    tok = torch.empty(B, Cn, T, **f)
    seq = torch.empty(B, Cn, **f)
    attn = _lib.XattnOut(probs.data_ptr() if want_probs else None, _p(layer), tsc.data_ptr() if want_scores else None,
                         psc.data_ptr() if want_scores else None)
    with torch.cuda.device(input_ids.device):
        rc = lib.gram_teacher_forced_ex(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, _ref(comp),
                                        decoder_input_ids.data_ptr(), labels.data_ptr(), Cn, T, workspace.data_ptr(), workspace.numel(),
                                        None, tok.data_ptr(), seq.data_ptr(), C.byref(attn), _stream(input_ids))
    _lib.check(rc, "gram_teacher_forced_ex")
    return probs, tsc, psc


@teacher_forced_attn.register_fake
def _(input_ids, attention_mask, handle, workspace, decoder_input_ids, labels, vocab_size, n_dec_layers, n_heads, want_probs, want_scores,
      comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L):
    B, N, L = input_ids.shape
    _, Cn, T = decoder_input_ids.shape
    Q, S = Cn * T, N * L
    f = dict(dtype=torch.float32)
    return (decoder_input_ids.new_empty((n_dec_layers, B, n_heads, Q, S) if want_probs else (0,), **f),
            decoder_input_ids.new_empty((B, Q, S) if want_scores else (0,), **f),
            decoder_input_ids.new_empty((B, Q, N) if want_scores else (0,), **f))


@torch.library.custom_op("gram::teacher_forced_scores", mutates_args=("workspace",), device_types="cuda")
def teacher_forced_scores(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, decoder_input_ids: Tensor,
                          labels: Tensor, vocab_size: int, comp_map: Optional[Tensor], comp_ids: Optional[Tensor],
                          comp_mask: Optional[Tensor], cache_slot: Optional[Tensor], cache_x: Optional[Tensor], n_cached: int,
                          cache_L: int) -> Tuple[Tensor, Tensor]:
    """The teacher-forced pass of ``teacher_forced`` (same inputs, validated by the same ``_tf_inputs``) with the cross-attention
    scores summed over heads inside the kernel (gram_teacher_forced_scores): no per-head buffer, any N*L the handle takes -- which
    must have been raised by gram_model_set_max_fused_len (GRAM_E_ARG otherwise).  Returns (token_scores f32 (B, C*T, N*L) = the
    probabilities summed over layers and heads, passage_scores f32 (B, C*T, N) = per passage the sum over its valid keys / (valid
    keys * n_dec_layers * n_heads), NaN for a passage without one)."""
    lib = _lib.load()
    B, N, L, Cn, T = _tf_inputs("teacher_forced_scores", input_ids, attention_mask, decoder_input_ids, labels, vocab_size)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    Q, S = Cn * T, N * L
    f = dict(dtype=torch.float32, device=input_ids.device)
    tsc = torch.empty(B, Q, S, **f)
    psc = torch.empty(B, Q, N, **f)
    tok = torch.empty(B, Cn, T, **f)
    seq = torch.empty(B, Cn, **f)
    out = _lib.XattnScores(tsc.data_ptr(), psc.data_ptr())
    with torch.cuda.device(input_ids.device):
        rc = lib.gram_teacher_forced_scores(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, _ref(comp),
                                            decoder_input_ids.data_ptr(), labels.data_ptr(), Cn, T, workspace.data_ptr(),
                                            workspace.numel(), None, tok.data_ptr(), seq.data_ptr(), C.byref(out), _stream(input_ids))
    _lib.check(rc, "gram_teacher_forced_scores")
    return tsc, psc


@teacher_forced_scores.register_fake
def _(input_ids, attention_mask, handle, workspace, decoder_input_ids, labels, vocab_size, comp_map, comp_ids, comp_mask, cache_slot,
      cache_x, n_cached, cache_L):
    B, N, L = input_ids.shape
    _, Cn, T = decoder_input_ids.shape
    f = dict(dtype=torch.float32)
    return (decoder_input_ids.new_empty(B, Cn * T, N * L, **f), decoder_input_ids.new_empty(B, Cn * T, N, **f))


# ---------------------------------------------------------------------------------------------- every item in one pass over the Trie
@torch.library.custom_op("gram::score_trie", mutates_args=("workspace",), device_types="cuda")
def score_trie(input_ids: Tensor, attention_mask: Tensor, handle: int, workspace: Tensor, trie_child_off: Tensor, trie_child_tok: Tensor,
               trie_child_node: Tensor, trie_max_fanout: int, trie_min_seq_len: int, row_tokens: Tensor, row_pos: Tensor, row_anc: Tensor,
               row_node: Tensor, node_row: Tensor, node_tok: Tensor, node_leaf: Tensor, n_leaves: int, vocab_size: int, want_nodes: bool,
               comp_map: Optional[Tensor], comp_ids: Optional[Tensor], comp_mask: Optional[Tensor], cache_slot: Optional[Tensor],
               cache_x: Optional[Tensor], n_cached: int, cache_L: int) -> Tuple[Tensor, Tensor]:
    """input_ids i64 (B,N,L), attention_mask u8 (B,N,L), ``handle`` a gram_model_t* as int, ``workspace`` a u8 scratch tensor of
    gram_workspace_bytes_trie; the Trie as its CSR arrays (gram_trie_t) and its row tables (gram_trie_rows_t,
    ``FlatTrie.decoder_rows``): row_tokens / row_pos / row_node i32 (Q,), row_anc i32 (Q, Tq), node_row / node_tok / node_leaf i32
    (n_nodes,); comp_* / cache_* the gram_compaction_t fields (None = off).  Returns (log p(item | user) f32 (B, n_leaves) by leaf
    rank, the per-edge terms f32 (B, n_nodes) by the node an edge enters -- empty unless want_nodes)."""
    lib = _lib.load()
    dev = input_ids.device
    if input_ids.dim() != 3 or row_anc.dim() != 2:
        raise ValueError("score_trie: input_ids must be (B, N, L) and row_anc (Q, Tq)")
    B, N, L = input_ids.shape
    Q, Tq = row_anc.shape
    n_nodes = trie_child_off.numel() - 1
    _check("input_ids", input_ids, torch.int64)
    _check("attention_mask", attention_mask, torch.uint8, (B, N, L), dev)
    for name, t, shape in (("trie_child_off", trie_child_off, None), ("trie_child_tok", trie_child_tok, None),
                           ("trie_child_node", trie_child_node, (trie_child_tok.numel(),)), ("row_tokens", row_tokens, (Q,)),
                           ("row_pos", row_pos, (Q,)), ("row_anc", row_anc, (Q, Tq)), ("row_node", row_node, (Q,)),
                           ("node_row", node_row, (n_nodes,)), ("node_tok", node_tok, (n_nodes,)), ("node_leaf", node_leaf, (n_nodes,))):
        _check(name, t, torch.int32, shape, dev)
    if Q < 1 or not 1 <= Tq <= _lib.GRAM_MAX_DEC_LEN or n_nodes < 3 or not 1 <= n_leaves < n_nodes:
        raise ValueError(f"score_trie: need Q >= 1 rows, 1 <= Tq <= {_lib.GRAM_MAX_DEC_LEN}, a Trie with a leaf (got Q={Q}, Tq={Tq}, "
                         f"n_nodes={n_nodes}, n_leaves={n_leaves})")
    # the tables index the embedding, the lm_head, the rows and the outputs on the device: out-of-range entries are refused here
    lim = torch.stack([row_tokens.min(), row_tokens.max(), row_pos.min(), row_pos.max(), row_anc.min(), row_anc.max(), row_node.min(),
                       row_node.max(), node_row.min(), node_row.max(), node_tok.min(), node_tok.max(), node_leaf.min(),
                       node_leaf.max()]).tolist()
    ok = (0 <= lim[0] and lim[1] < vocab_size and 0 <= lim[2] and lim[3] < Tq and 0 <= lim[4] and lim[5] < Q and 0 <= lim[6]
          and lim[7] < n_nodes and -1 <= lim[8] and lim[9] < Q and -1 <= lim[10] and lim[11] < vocab_size and -1 <= lim[12]
          and lim[13] < n_leaves)
    if not ok:
        raise ValueError("score_trie: a row table entry is out of range (tokens in [0, vocab), pos in [0, Tq), anc in [0, Q), "
                         "row_node in [0, n_nodes), node_row in [-1, Q), node_tok in [-1, vocab), node_leaf in [-1, n_leaves))")
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len)
    rows = _lib.TrieRows(row_tokens.data_ptr(), row_pos.data_ptr(), row_anc.data_ptr(), row_node.data_ptr(), node_row.data_ptr(),
                         node_tok.data_ptr(), node_leaf.data_ptr(), Q, Tq, n_nodes, n_leaves)
    comp = _compaction(comp_map, comp_ids, comp_mask, cache_slot, cache_x, n_cached, cache_L)
    leaf = torch.empty(B, n_leaves, dtype=torch.float32, device=dev)
    nodes = torch.empty((B, n_nodes) if want_nodes else (0,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gram_score_trie(handle, input_ids.data_ptr(), attention_mask.data_ptr(), B, N, L, _ref(comp), C.byref(trie),
                                 C.byref(rows), workspace.data_ptr(), workspace.numel(), leaf.data_ptr(),
                                 nodes.data_ptr() if want_nodes else None, _stream(input_ids))
    _lib.check(rc, "gram_score_trie")
    return leaf, nodes


@score_trie.register_fake
def _(input_ids, attention_mask, handle, workspace, trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, trie_min_seq_len,
      row_tokens, row_pos, row_anc, row_node, node_row, node_tok, node_leaf, n_leaves, vocab_size, want_nodes, comp_map, comp_ids,
      comp_mask, cache_slot, cache_x, n_cached, cache_L):
    B = input_ids.shape[0]
    f = dict(dtype=torch.float32)
    return (input_ids.new_empty(B, n_leaves, **f), input_ids.new_empty((B, trie_child_off.numel() - 1) if want_nodes else (0,), **f))


# ---------------------------------------------------------------------------------------------- linear
@torch.library.custom_op("gram::linear", mutates_args=(), device_types="cuda")
def linear(a: Tensor, w: Tensor, relu: bool = False) -> Tensor:
    """a (M, K) row-major (rows may be strided: stride(1) == 1, stride(0) % 8 == 0), w (N, K) contiguous ([out][in], as nn.Linear
    stores it), both of the library's 16-bit type (_lib.piece_dtype()): (M, N) = a @ w^T, fp32 accumulate.  N % 128 == 0, K % 64 == 0."""
    dt = _lib.piece_dtype()
    if a.dim() != 2 or w.dim() != 2:
        raise ValueError("linear: a must be (M, K) and w (N, K)")
    M, K = a.shape
    N = w.shape[0]
    _check("a", a, dt, contiguous=False)
    _check("w", w, dt, (None, K), a.device)
    if M < 1 or a.stride(1) != 1 or a.stride(0) < K or a.stride(0) % 8 or N % 128 or K % 64:
        raise ValueError(f"linear: need M >= 1, a.stride(1) == 1, a.stride(0) >= K and % 8 == 0, N % 128 == 0, K % 64 == 0 "
                         f"(got a {tuple(a.shape)} strides {a.stride()}, w {tuple(w.shape)})")
    out = torch.empty(M, N, dtype=dt, device=a.device)
    with torch.cuda.device(a.device):
        rc = _lib.load().gram_gemm_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, a.stride(0), N,
                                        _lib.EPI_BF16_RELU if relu else _lib.EPI_BF16, None, _stream(a))
    _lib.check(rc, "gram_gemm_bf16")
    return out


@linear.register_fake
def _(a, w, relu=False):
    return a.new_empty(a.shape[0], w.shape[0])


# ---------------------------------------------------------------------------------------------- encoder self-attention
def _enc_self_attn(op: str, max_len: int, fn: str, qkv: Tensor, bias: Tensor, mask: Tensor, num_heads: int, *pieces) -> Tensor:
    """Both encoder self-attention ops: passages of up to ``max_len`` tokens through the C call ``fn``, whose piece arguments (the
    split form's) are ``pieces``."""
    dt = _lib.piece_dtype()
    if mask.dim() != 2:
        raise ValueError(f"{op}: mask must be (P, L)")
    P, L = mask.shape
    inner = num_heads * 64
    _check("qkv", qkv, dt, (P * L, 3 * inner))
    _check("bias", bias, torch.float32, (num_heads, 255), qkv.device)
    _check("mask", mask, torch.uint8, None, qkv.device)
    if L < 32 or L > max_len or L % 32 or num_heads < 1:
        raise ValueError(f"{op}: L must be a multiple of 32 in [32, {max_len}] (got {L})")
    out = torch.empty(P * L, inner, dtype=dt, device=qkv.device)
    with torch.cuda.device(qkv.device):
        rc = getattr(_lib.load(), fn)(qkv.data_ptr(), bias.data_ptr(), mask.data_ptr(), out.data_ptr(), P, L, num_heads, *pieces,
                                      _stream(qkv))
    _lib.check(rc, fn)
    return out


def _enc_self_attn_fake(qkv, bias, mask, num_heads):
    return qkv.new_empty(qkv.shape[0], num_heads * 64)


@torch.library.custom_op("gram::enc_self_attn", mutates_args=(), device_types="cuda")
def enc_self_attn(qkv: Tensor, bias: Tensor, mask: Tensor, num_heads: int) -> Tensor:
    """qkv 16-bit (P*L, 3*inner) rows q|k|v; bias f32 (H, 255) by (key - query + 127); mask u8 (P, L) -> 16-bit (P*L, inner)."""
    return _enc_self_attn("enc_self_attn", _lib.GRAM_MAX_PASSAGE_LEN, "gram_enc_self_attn", qkv, bias, mask, num_heads)


@torch.library.custom_op("gram::enc_self_attn_long", mutates_args=(), device_types="cuda")
def enc_self_attn_long(qkv: Tensor, bias: Tensor, mask: Tensor, num_heads: int) -> Tensor:
    """``enc_self_attn`` for passages of up to 512 tokens (gram_enc_self_attn_long_split, one piece): the same operands; the bias
    index is clamp(key - query, -127, 127) + 127, so the (H, 255) table must be constant beyond +-127."""
    return _enc_self_attn("enc_self_attn_long", _lib.GRAM_MAX_LONG_PASSAGE_LEN, "gram_enc_self_attn_long_split", qkv, bias, mask,
                          num_heads, 1, 0)


enc_self_attn.register_fake(_enc_self_attn_fake)
enc_self_attn_long.register_fake(_enc_self_attn_fake)


# ---------------------------------------------------------------------------------------------- cross-attention decode
def _cross_attn_inputs(op: str, max_keys: int, q: Tensor, k_bank: Tensor, vt_bank: Tensor, mask: Tensor,
                       num_beams: int) -> Tuple[int, int, int]:
    """What both cross-attention ops require of their operands, over up to ``max_keys`` keys; returns (B, H, S)."""
    dt = _lib.piece_dtype()
    if k_bank.dim() != 4 or k_bank.shape[-1] != 64:
        raise ValueError(f"{op}: k_bank must be (B, H, S, 64)")
    B, H, S, _ = k_bank.shape
    if S < 32 or S % 32 or S > max_keys or not 1 <= num_beams <= _lib.GRAM_MAX_BEAMS:
        raise ValueError(f"{op}: S must be a multiple of 32 in [32, {max_keys}] and 1 <= num_beams <= {_lib.GRAM_MAX_BEAMS}")
    _check("k_bank", k_bank, dt)
    _check("vt_bank", vt_bank, dt, (B, H, S // 32, 64, 32), k_bank.device)  # V^T blocked by 32 keys
    _check("q", q, dt, (B * num_beams, H * 64), k_bank.device)
    _check("mask", mask, torch.uint8, (B, S), k_bank.device)
    return B, H, S


def _cross_attn_fake(q, k_bank, vt_bank, mask, num_beams):
    return torch.empty_like(q)


@torch.library.custom_op("gram::cross_attn_decode", mutates_args=(), device_types="cuda")
def cross_attn_decode(q: Tensor, k_bank: Tensor, vt_bank: Tensor, mask: Tensor, num_beams: int) -> Tensor:
    """q bf16 (B*K, inner); k_bank bf16 (B, H, S, 64); vt_bank bf16 (B, H, S/32, 64, 32) = V transposed, blocked by 32 keys (one
    copy per user, shared by its K beams); mask u8 (B, S) -> bf16 (B*K, inner)."""
    B, H, S = _cross_attn_inputs("cross_attn_decode", _lib.GRAM_MAX_FUSED_LEN, q, k_bank, vt_bank, mask, num_beams)
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        rc = _lib.load().gram_cross_attn_decode(q.data_ptr(), k_bank.data_ptr(), vt_bank.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                                B, num_beams, H, S, _stream(q))
    _lib.check(rc, "gram_cross_attn_decode")
    return out


@torch.library.custom_op("gram::cross_attn_long", mutates_args=(), device_types="cuda")
def cross_attn_long(q: Tensor, k_bank: Tensor, vt_bank: Tensor, mask: Tensor, num_beams: int) -> Tensor:
    """``cross_attn_decode`` over up to 16 384 fused keys (gram_mask_key_bits_long + gram_cross_attn_long_split, one piece): the same
    operands.  A row's bits depend on the query row and the user's valid 32-key steps in order, not on the batch or on S; they are
    not ``cross_attn_decode``'s bits (another summation order)."""
    B, H, S = _cross_attn_inputs("cross_attn_long", _lib.GRAM_MAX_LONG_FUSED_LEN, q, k_bank, vt_bank, mask, num_beams)
    lib = _lib.load()
    out = torch.empty_like(q)
    bits = torch.empty(B, _lib.GRAM_KEY_BITS_LONG_STRIDE, dtype=torch.int32, device=q.device)
    scratch = torch.empty(max(1, int(lib.gram_cross_attn_long_scratch_bytes(B * num_beams, H, S)) // 4), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(lib.gram_mask_key_bits_long(mask.data_ptr(), bits.data_ptr(), B, S, _stream(q)), "gram_mask_key_bits_long")
        rc = lib.gram_cross_attn_long_split(q.data_ptr(), k_bank.data_ptr(), vt_bank.data_ptr(), mask.data_ptr(), out.data_ptr(), B, num_beams,
                                            H, S, None, None, 1, 0, 0, bits.data_ptr(), scratch.data_ptr(), _stream(q))
    _lib.check(rc, "gram_cross_attn_long_split")
    return out


cross_attn_decode.register_fake(_cross_attn_fake)
cross_attn_long.register_fake(_cross_attn_fake)


# ---------------------------------------------------------------------------------------------- Trie-constrained search step
@torch.library.custom_op("gram::trie_step", mutates_args=("tokens", "node", "beam_scores", "seq", "anc", "done", "n_hyps", "hyp_score",
                                                          "worst", "hyp_len", "hyp_tok", "error"), device_types="cuda")
def trie_step(logits: Tensor, tokens: Tensor, node: Tensor, beam_scores: Tensor, seq: Tensor, anc: Tensor, done: Tensor,
              n_hyps: Tensor, hyp_score: Tensor, worst: Tensor, hyp_len: Tensor, hyp_tok: Tensor, error: Tensor,
              trie_child_off: Tensor, trie_child_tok: Tensor, trie_child_node: Tensor, trie_max_fanout: int, num_beams: int,
              cur_len: int, length_penalty: float) -> Tensor:
    """One HF-4.26 beam-search step on dense logits f32 (B*K, V): log-softmax normaliser, Trie mask, top-2K, BeamSearchScorer.process,
    the beam state (gram_beam_state_t fields) advanced in place.  Returns the row LSE f32 (B*K)."""
    lib = _lib.load()
    if logits.dim() != 2 or seq.dim() != 2:
        raise ValueError("trie_step: logits must be (B*K, V) and seq (B*K, Tmax)")
    R, V = logits.shape
    K = num_beams
    if K < 1 or K > _lib.GRAM_MAX_BEAMS or R % K or not 1 <= cur_len < seq.shape[1] or seq.shape[1] > _lib.GRAM_MAX_DEC_LEN:
        raise ValueError("trie_step: rows must be B * num_beams, 1 <= cur_len < Tmax <= %d" % _lib.GRAM_MAX_DEC_LEN)
    Bq, Tq, dev = R // K, seq.shape[1], logits.device
    _check("logits", logits, torch.float32)
    for name, t, dtype, shape in (("tokens", tokens, torch.int32, (R,)), ("node", node, torch.int32, (R,)),
                                  ("beam_scores", beam_scores, torch.float32, (R,)), ("seq", seq, torch.int32, (R, Tq)),
                                  ("anc", anc, torch.int32, (Tq, R)), ("done", done, torch.int32, (Bq,)),
                                  ("n_hyps", n_hyps, torch.int32, (Bq,)), ("hyp_score", hyp_score, torch.float64, (Bq, K + 1)),
                                  ("worst", worst, torch.float64, (Bq,)), ("hyp_len", hyp_len, torch.int32, (Bq, K + 1)),
                                  ("hyp_tok", hyp_tok, torch.int32, (Bq, K + 1, Tq)), ("error", error, torch.int32, None),
                                  ("trie_child_off", trie_child_off, torch.int32, None),
                                  ("trie_child_tok", trie_child_tok, torch.int32, None),
                                  ("trie_child_node", trie_child_node, torch.int32, (trie_child_tok.numel(),))):
        _check(name, t, dtype, shape, dev)
    if error.numel() < 1 or trie_child_off.numel() < 2:
        raise ValueError("trie_step: error needs >= 1 element, trie_child_off >= 2")
    st = _lib.BeamState(B=R // K, K=K, Tmax=seq.shape[1], length_penalty=length_penalty, eos=1, pad=0, tokens=tokens.data_ptr(),
                        node=node.data_ptr(), beam_scores=beam_scores.data_ptr(), seq=seq.data_ptr(), anc=anc.data_ptr(),
                        done=done.data_ptr(), n_hyps=n_hyps.data_ptr(), hyp_score=hyp_score.data_ptr(), worst=worst.data_ptr(),
                        hyp_len=hyp_len.data_ptr(), hyp_tok=hyp_tok.data_ptr(), error=error.data_ptr())
    trie = _trie(trie_child_off, trie_child_tok, trie_child_node, trie_max_fanout, 0)  # (a dense step has no minimum length)
    lse = torch.empty(R, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        _lib.check(lib.gram_row_lse(logits.data_ptr(), lse.data_ptr(), R, V, _stream(logits)), "gram_row_lse")
        _lib.check(lib.gram_beam_step(C.byref(st), C.byref(trie), logits.data_ptr(), lse.data_ptr(), V, cur_len, K, _stream(logits)),
                   "gram_beam_step")
    return lse


@trie_step.register_fake
def _(logits, tokens, node, beam_scores, seq, anc, done, n_hyps, hyp_score, worst, hyp_len, hyp_tok, error, trie_child_off,
      trie_child_tok, trie_child_node, trie_max_fanout, num_beams, cur_len, length_penalty):
    return logits.new_empty(logits.shape[0])


# (``sample`` / ``sample_items`` are reached as torch.ops.gram.* like the rest; their schemas are pinned by tests/test_sample_host.py, the
# twelve names below by tests/test_ops_host.py, which counts them)
__all__ = ["generate", "generate_items", "teacher_forced", "teacher_forced_attn", "teacher_forced_scores", "score_trie", "linear", "enc_self_attn", "enc_self_attn_long", "cross_attn_decode", "cross_attn_long", "trie_step"]
