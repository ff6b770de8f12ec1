"""Generation over a static KV cache (harness.py re-exports it): DecodeCache, DecodeSession and `generate`, model.generate's counterpart
for an unpadded batch on the GPU.  Depends on runtime.py only; transformers is imported on first use."""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn

from . import runtime

# The HIP decode attention in folded layers (fusion._folded_layer_forward) over a DecodeCache.  False: those layers append to the
# cache and attend through HF's StaticLayer.update and attention interface instead (tools/bench_generate.py compares the two).  Read
# HERE when a step runs or is captured: nothing re-exports it.
DECODE_ATTENTION = True
# The HIP causal prefill attention in folded layers for MORE than 4 rows over a DecodeCache (runtime.prefill_attention_f16).  False (the
# default): those calls run LlamaDecoderLayer.forward -- StaticLayer.update and HF's attention interface over the whole cache
# (tools/bench_prefill_attention.py compares the two).  Read HERE when a forward runs.
PREFILL_ATTENTION = False
_DECODE_CACHE = None                    # the DecodeCache class, made on first use (transformers is imported lazily)
_KV8_LAYER = None                       # the FP8 cache's layer class, likewise
KV_CACHE_FORMATS = ("fp16", "fp8")      # DecodeSession(..., kv_cache=) / generate(..., kv_cache=)


def _decode_cache_layer(cache, layer_idx: int, batch: int, n_kv: int, head_dim: int):
    """the StaticLayer of `cache` that the decode-attention branch may append to and attend over: cache is a DecodeCache, its layer
    is a plain, initialised StaticLayer of fp16 [batch, n_kv, max_len, head_dim] tensors -- else None (HF's path)"""
    if not DECODE_ATTENTION or _DECODE_CACHE is None or not isinstance(cache, _DECODE_CACHE) or layer_idx is None \
            or layer_idx >= len(cache.layers):
        return None
    from transformers.cache_utils import StaticLayer
    lay = cache.layers[layer_idx]
    if type(lay) is not StaticLayer or not lay.is_initialized or lay.keys.dtype != torch.float16:
        return None
    B, H, L, D = lay.keys.shape
    if (B, H, D) != (batch, n_kv, head_dim) or not runtime.decode_attention_ok(batch, 1, n_kv, n_kv, head_dim, L):
        return None
    return lay


def _prefill_cache_layer(cache, layer_idx: int, batch: int, seq: int, n_q: int, n_kv: int, head_dim: int, branch: bool = False):
    """_decode_cache_layer's counterpart for the prefill-attention branch (any batch, any number of rows): cache is a DecodeCache, its
    layer a plain, initialised StaticLayer of fp16 [batch, n_kv, max_len, head_dim] tensors that runtime.prefill_attention_ok takes
    -- else None (HF's path).  branch: the cache carries a branch table (_cache_branch): PREFILL_ATTENTION is not asked"""
    if not (PREFILL_ATTENTION or branch) or _DECODE_CACHE is None or not isinstance(cache, _DECODE_CACHE) or layer_idx is None \
            or layer_idx >= len(cache.layers):
        return None
    from transformers.cache_utils import StaticLayer
    lay = cache.layers[layer_idx]
    if type(lay) is not StaticLayer or not lay.is_initialized or lay.keys.dtype != torch.float16:
        return None
    B, H, L, D = lay.keys.shape
    if (B, H, D) != (batch, n_kv, head_dim) or not runtime.prefill_attention_ok(batch, seq, n_q, n_kv, head_dim, L):
        return None
    return lay


def _cache_branch(cache):
    """(trunk, lo), the branch table a scorer has set on a DecodeCache around one forward (scoring.loglikelihood(share_prefix=True);
    runtime.branch_attention_f16's tables) -- else None"""
    if _DECODE_CACHE is None or not isinstance(cache, _DECODE_CACHE):
        return None
    return cache.branch


def _kv8_cache_layer(cache, layer_idx: int):
    """the FP8 layer of `cache` for decoder layer layer_idx (DecodeCache(..., kv_cache="fp8")) -- else None.  A folded layer that finds
    one appends and attends with the FP8 entries (runtime.rope_append_kv8 / decode_attention_kv8 / prefill_attention_kv8) whatever
    DECODE_ATTENTION and PREFILL_ATTENTION say: HF's attention cannot read this cache, so there is no other path."""
    if _KV8_LAYER is None or _DECODE_CACHE is None or not isinstance(cache, _DECODE_CACHE) or layer_idx is None \
            or layer_idx >= len(cache.layers):
        return None
    lay = cache.layers[layer_idx]
    return lay if type(lay) is _KV8_LAYER and lay.is_initialized else None


def _kv8_layer_class():
    global _KV8_LAYER
    if _KV8_LAYER is None:
        from transformers.cache_utils import StaticLayer

        class Kv8StaticLayer(StaticLayer):
            """A StaticLayer whose rows are FP8 (the format: runtime.kv8_quantize): keys / values uint8 [B, Hkv, max_len, D] with one
            fp32 power-of-two scale per row in key_scales / value_scales [B, Hkv, max_len].  cumulative_length, get_seq_length, the
            mask helpers and reset work as in StaticLayer; update() raises, because HF's attention cannot read these rows -- only
            folded layers (fuse_decode_(epilogues=True)) append to and attend over it.  runtime.kv8_dequantize(lay.keys,
            lay.key_scales) shows what it holds."""

            def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
                self.dtype, self.device = torch.uint8, key_states.device
                self.batch_size, self.num_heads = key_states.shape[:2]
                self.k_head_dim = self.v_head_dim = key_states.shape[-1]
                rows = (self.batch_size, self.num_heads, self.max_cache_len)
                self.keys = torch.zeros(*rows, self.k_head_dim, dtype=torch.uint8, device=self.device)
                self.values = torch.zeros(*rows, self.v_head_dim, dtype=torch.uint8, device=self.device)
                self.key_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
                self.value_scales = torch.zeros(rows, dtype=torch.float32, device=self.device)
                self.cumulative_length = self.cumulative_length.to(self.device)
                self.is_initialized = True

            def update(self, key_states, value_states, *args, **kwargs):
                raise RuntimeError("the FP8 KV cache is written by the HIP entries of folded layers (fuse_decode_(epilogues=True)) only: "
                                   "StaticLayer.update / HF's attention cannot use it")

            def reset(self) -> None:
                super().reset()
                if self.is_initialized:
                    self.key_scales.zero_()
                    self.value_scales.zero_()

        Kv8StaticLayer.__qualname__ = "Kv8StaticLayer"
        _KV8_LAYER = Kv8StaticLayer
    return _KV8_LAYER


def _kv8_refusal(model: nn.Module, batch: int, max_length: int) -> str | None:
    """why DecodeSession(model, batch, max_length, kv_cache="fp8") cannot run -- the first condition that fails -- or None"""
    from . import fusion
    try:
        from transformers.models.llama.modeling_llama import LlamaDecoderLayer
    except ImportError:
        return "transformers' LLaMA model is not importable"
    layers = [m for m in model.modules() if isinstance(m, LlamaDecoderLayer)]
    cfg = model.config.get_text_config(decoder=True)
    if not layers or len(layers) != cfg.num_hidden_layers \
            or not all(getattr(lay.forward, "__func__", None) is fusion._folded_layer_forward for lay in layers):
        return "every decoder layer must be a folded layer of fuse_decode_(model, epilogues=True): no other layer can read this cache"
    if model.get_input_embeddings().weight.dtype != torch.float16:
        return "the model must be fp16"
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    if head_dim not in (64, 128):
        return f"head_dim must be 64 or 128, not {head_dim}"
    if batch > 4:
        return f"batch must be at most 4, not {batch}"
    if max_length > 65536:
        return f"max_length must be at most 65536, not {max_length}"
    if not runtime.kv8_ok(batch, 1, cfg.num_attention_heads, cfg.num_key_value_heads, head_dim, max_length):
        return "runtime.kv8_ok declines these heads"
    return None


def _decode_cache_class():
    global _DECODE_CACHE
    if _DECODE_CACHE is None:
        from transformers.cache_utils import StaticCache, StaticLayer

        class DecodeCache(StaticCache):
            """transformers' StaticCache for an UNPADDED batch whose rows all share one position, allocated up front (so that a
            decode step can be captured before any row is written).  Made by DecodeSession / generate, not by the user.  HF code
            that receives it treats it as a StaticCache: StaticLayer.update, prefill of more than 4 rows, unfolded layers and bf16
            models keep working.  A folded layer (fuse_decode_(epilogues=True)) whose cache layer is a plain fp16 StaticLayer
            appends to it and attends over its valid rows with the HIP decode attention (runtime.rope_append_f16 /
            decode_attention_f16) instead -- and, with PREFILL_ATTENTION on, a prefill of more than 4 rows with
            runtime.prefill_attention_f16; those paths ignore the attention mask, hence the unpadded-batch contract.
            kv_cache="fp8": every layer is a Kv8StaticLayer instead -- half the bytes, for folded layers only (DecodeSession checks).
            branch: normally None.  scoring.loglikelihood(share_prefix=True) sets (trunk, lo) -- runtime.branch_attention_f16's tables
            for the rows of the NEXT forward -- around one forward and clears it in a finally; folded layers then attend with
            runtime.branch_attention_f16 whatever the row count, and a layer that cannot raises."""

            def __init__(self, config, batch: int, max_cache_len: int, device, dtype, kv_cache: str = "fp16"):
                super().__init__(config=config, max_cache_len=max_cache_len)
                if kv_cache not in KV_CACHE_FORMATS:
                    raise ValueError(f"DecodeCache: kv_cache must be one of {KV_CACHE_FORMATS}, not {kv_cache!r}")
                self.kv_cache = kv_cache
                if kv_cache == "fp8":
                    if not all(type(lay) is StaticLayer for lay in self.layers):
                        raise ValueError("DecodeCache: the FP8 cache replaces plain StaticLayers only (no sliding-window layers)")
                    self.layers = [_kv8_layer_class()(max_cache_len=max_cache_len) for _ in self.layers]
                text = config.get_text_config(decoder=True)
                head_dim = getattr(text, "head_dim", None) or text.hidden_size // text.num_attention_heads
                self.early_initialization(batch, text.num_key_value_heads, head_dim, dtype, torch.device(device))
                self.batch = batch
                self.branch = None

        DecodeCache.__qualname__ = "DecodeCache"
        _DECODE_CACHE = DecodeCache
    return _DECODE_CACHE


def _capture_graph(unit, device, restore=(), warmup: int = 2):
    """Warm `unit` up on a side stream (after every run the tensors in `restore` get their values back), then capture ONE run of it
    in a hipGraph -- the capture runs nothing.  Returns (graph, what unit returned under capture)"""
    # The collector stays off while the unit is warmed up and captured.  Seen once: the GPU test process aborted (SIGABRT, main thread,
    # "Garbage-collecting" in the dump) at a pure-Python line of a forward over the FP8 cache, in a suite whose earlier tests had left
    # torch.profiler results behind -- reference cycles of thousands of objects that only the collector frees.  The destructor that
    # aborted was not identified and the abort was not reproduced; torch.cuda.graph does not collect before it captures any more, so a
    # finaliser can run in the middle of a capture.  This closes that window at no cost (nothing is collected here).
    import gc
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        saved = [t.clone() for t in restore]
        s = torch.cuda.Stream(device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                unit()
                for t, v in zip(restore, saved):
                    t.copy_(v)
        torch.cuda.current_stream(device).wait_stream(s)
        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            out = unit()
    finally:
        if was_enabled:
            gc.enable()
    return graph, out


@dataclass
class _Selection:
    """DecodeSession.begin_selection's state: prompt in columns [0, col0) of `tokens`, n tokens wanted, `done` so far; params (T, k, p);
    processors (repetition_penalty, no_repeat_ngram_size, min_new_tokens, min_length) with `process`: whether one of them can act, i.e.
    whether a step runs pbl_process_logits_f16 at all; `scratch` fp16 [batch, total] for the penalty"""
    tokens: torch.Tensor
    col0: int
    n: int
    done: int
    uniforms: torch.Tensor | None
    pad: int
    eos: torch.Tensor | None
    step: torch.Tensor
    unfinished: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor
    params: tuple[float, int, float]
    min_p: float = 0.0
    processors: tuple[float, int, int, int] = (1.0, 0, 0, 0)
    process: bool = False
    scratch: torch.Tensor | None = None


@dataclass
class _Speculation:
    """DecodeSession.begin_speculation's state: prompt in columns [0, col0) of `tokens`, K drafts per step from n-grams of at most
    max_ngram tokens; `state` holds [cursor, unfinished count] as two int64 words (ONE device read per poll): `cursor` is a view of the
    first, `count` an int32 view of the low half of the second"""
    tokens: torch.Tensor
    col0: int
    total: int
    K: int
    max_ngram: int
    pad: int
    eos: torch.Tensor | None
    ids: torch.Tensor
    state: torch.Tensor
    cursor: torch.Tensor
    count: torch.Tensor
    unfinished: torch.Tensor
    status: torch.Tensor
    stats: torch.Tensor
    positions: torch.Tensor
    polls: int = 0


class DecodeSession:
    """Decoding state of `model` (a HF causal LM) for `batch` unpadded rows and at most `max_length` positions: a DecodeCache
    on the device and, with graph=True, ONE decode step captured in a hipGraph on its first call and replayed for every later
    token.  Every forward gets a ready 4D causal mask built on the device from the cache's position (create_causal_mask passes a
    4D mask through), so nothing in a step reads the position on the host.  The host keeps its own count (`pos`) to enforce
    max_length.

    prefill / step hand the logits back and leave the choice of the token to the caller.  begin_selection / select / step_select
    keep the choice on the device as well (runtime.select_token_f16: greedy or temperature / top-k / top-p / min-p sampling, eos /
    pad bookkeeping): the captured unit is then "forward over static_ids, select into static_ids", and a generation is one replay per
    token with nothing read on the host (run_selection reads the unfinished count every poll_every tokens).  A selection begun with
    a repetition penalty, a no-repeat n-gram size or a minimum length runs runtime.process_logits_f16 on the logits in front of the
    selection, inside the same unit; one begun without them launches exactly what it launched before they existed.

    begin_speculation / step_speculate / run_speculation decode greedily 1 + K tokens per row and step (prompt-lookup speculative
    decoding): the unit is "forward over the last token and K drafts, verify, draft" (runtime.spec_verify_f16), captured once.

    kv_cache="fp8": the cache rows are FP8 with one power-of-two scale each (runtime.kv8_quantize), half the bytes of the fp16 cache.
    Only the HIP entries of folded layers read such a cache, so the constructor raises ValueError -- naming the first condition that
    fails -- unless every decoder layer is a fuse_decode_(epilogues=True) folded layer, the model is fp16, head_dim is 64 or 128,
    batch <= 4 and max_length <= 65536.  Everything above works unchanged over it."""

    def __init__(self, model: nn.Module, batch: int, max_length: int, graph: bool = True, kv_cache: str = "fp16"):
        if batch < 1 or max_length < 1:
            raise ValueError("DecodeSession: batch and max_length must be >= 1")
        if kv_cache not in KV_CACHE_FORMATS:
            raise ValueError(f"DecodeSession: kv_cache must be one of {KV_CACHE_FORMATS}, not {kv_cache!r}")
        if kv_cache == "fp8":
            why = _kv8_refusal(model, int(batch), int(max_length))
            if why is not None:
                raise ValueError(f'DecodeSession: kv_cache="fp8": {why}')
        emb = model.get_input_embeddings().weight
        self.model, self.batch, self.max_length, self.use_graph = model, int(batch), int(max_length), graph
        self.device, self.dtype, self.kv_cache = emb.device, emb.dtype, kv_cache
        self.cache = _decode_cache_class()(model.config, self.batch, self.max_length, self.device, self.dtype, kv_cache=kv_cache)
        self._cols = torch.arange(self.max_length, device=self.device)
        self._bool_mask = model.config._attn_implementation == "sdpa"
        self.static_ids = torch.zeros(self.batch, 1, dtype=torch.long, device=self.device)
        self.graph, self.static_logits, self.sel, self.sel_graph, self.pos = None, None, None, None, 0
        self.spec, self.spec_graph = None, None

    def _mask(self, seq: int) -> torch.Tensor:
        """[batch, 1, seq, max_length]: query row s sees cache rows [0, position + s] (bool for SDPA, additive otherwise)"""
        rows = self.cache.layers[0].cumulative_length + torch.arange(seq, device=self.device)
        m = (self._cols[None, :] <= rows[:, None])[None, None].expand(self.batch, 1, seq, self.max_length)
        if self._bool_mask:
            return m
        return torch.zeros((), dtype=self.dtype, device=self.device).masked_fill(~m, torch.finfo(self.dtype).min)

    def _forward(self, ids: torch.Tensor) -> torch.Tensor:
        out = self.model(ids, attention_mask=self._mask(ids.shape[1]), past_key_values=self.cache, use_cache=True, logits_to_keep=1)
        return out.logits[:, -1]

    def _advance(self, seq: int):
        if self.pos + seq > self.max_length:
            raise ValueError(f"DecodeSession: {self.pos} + {seq} positions exceed max_length = {self.max_length}")
        self.pos += seq

    @torch.no_grad()
    def prefill(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [batch, S] at the current position, eagerly (<= 4 rows in folded layers: the HIP kernels; more: HF's StaticLayer.update
        and attention, or with PREFILL_ATTENTION the HIP prefill attention).  Returns the last position's logits [batch, vocab]."""
        if ids.dim() != 2 or ids.shape[0] != self.batch or ids.shape[1] < 1:
            raise ValueError(f"DecodeSession.prefill: ids must be [{self.batch}, S >= 1]")
        self._advance(ids.shape[1])
        return self._forward(ids.to(self.device))

    @torch.no_grad()
    def step(self, tok: torch.Tensor) -> torch.Tensor:
        """one token per row (tok [batch] or [batch, 1]) at the current position; returns the logits [batch, vocab] -- with
        graph=True a view of the graph's static output, overwritten by the next step"""
        if tok.numel() != self.batch:
            raise ValueError(f"DecodeSession.step: one token per row ({self.batch})")
        self._advance(1)
        if not self.use_graph:
            return self._forward(tok.reshape(self.batch, 1).to(self.device))
        self.static_ids.copy_(tok.reshape(self.batch, 1))
        if self.graph is None:
            self.graph, self.static_logits = self._capture(lambda: self._forward(self.static_ids))
        self.graph.replay()
        return self.static_logits

    def _capture(self, unit, state=()):
        """_capture_graph of `unit`: its warm-up writes this position's rows, which the replay rewrites; its position advance and what
        it did to the tensors in `state` are undone"""
        return _capture_graph(unit, self.device, [lay.cumulative_length for lay in self.cache.layers] + list(state))

    # ---- token selection on the device
    def begin_selection(self, prompt: torch.Tensor, total: int, eos=(), pad: int | None = None, uniforms: torch.Tensor | None = None,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0,
                        no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, min_length: int = 0, min_p: float = 0.0) -> torch.Tensor:
        """Start a generation whose tokens are chosen on the device: allocates the result `tokens` [batch, total] (int64, the
        prompt [batch, P] in front, returned), the step counter, the rows' unfinished flags, their count and the status word.
        uniforms None: greedy; else fp32 [>= total - P, batch] uniforms in [0, 1), row t for the t-th new token, with temperature /
        top_k (0 = off) / top_p (1 = off) / min_p (0 = off).  eos: ids that finish a row (finished rows receive `pad`).
        repetition_penalty (1 = off), no_repeat_ngram_size (0 = off, at most 8), min_new_tokens / min_length (eos ids blocked while
        fewer than min_new_tokens new tokens or min_length tokens in all exist): HF's processors of those names, applied to the
        logits by runtime.process_logits_f16 before every selection -- greedy or sampled; the penalty's scratch is allocated here."""
        if prompt.dim() != 2 or prompt.shape[0] != self.batch or not prompt.shape[1] < total:
            raise ValueError(f"DecodeSession.begin_selection: prompt must be [{self.batch}, P < total]")
        if not repetition_penalty > 0 or not 0 <= no_repeat_ngram_size <= runtime.PROCESS_MAX_NGRAM or not 0 <= min_p <= 1:
            raise ValueError(f"DecodeSession.begin_selection: repetition_penalty > 0, 0 <= no_repeat_ngram_size <= "
                             f"{runtime.PROCESS_MAX_NGRAM} and 0 <= min_p <= 1")
        dev, P = self.device, int(prompt.shape[1])
        if uniforms is not None:
            if uniforms.dim() != 2 or uniforms.shape[0] < total - P or uniforms.shape[1] != self.batch:
                raise ValueError(f"DecodeSession.begin_selection: uniforms must be [>= {total - P}, {self.batch}]")
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        tokens = torch.zeros(self.batch, total, dtype=torch.long, device=dev)
        tokens[:, :P] = prompt
        eos = [int(e) for e in eos]
        self.sel = _Selection(tokens=tokens, col0=P, n=int(total) - P, done=0, uniforms=uniforms, pad=0 if pad is None else int(pad),
                              eos=torch.tensor(eos, dtype=torch.long, device=dev) if eos else None,
                              step=torch.zeros(1, dtype=torch.long, device=dev), unfinished=torch.ones(self.batch, dtype=torch.bool, device=dev),
                              count=torch.full((1,), self.batch, dtype=torch.int32, device=dev),
                              status=torch.zeros(1, dtype=torch.int32, device=dev), params=(float(temperature), int(top_k), float(top_p)),
                              min_p=float(min_p))
        theta, ngram, min_new, min_len = float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens), int(min_length)
        c = self.sel
        c.processors = (theta, ngram, min_new, min_len)
        c.process = theta != 1.0 or ngram > 0 or (bool(eos) and (min_new > 0 or min_len > P))
        if theta != 1.0:
            c.scratch = torch.empty(self.batch, total, dtype=torch.float16, device=dev)
        self.sel_graph = None                                 # a captured unit holds the previous selection's tensors and parameters
        return tokens

    @torch.no_grad()
    def select(self, logits: torch.Tensor) -> None:
        """choose the next token of every row from `logits` [batch, vocab] fp16 on the device: it lands in the result, in static_ids
        (the next step's input) and in the bookkeeping of begin_selection.  With processors (begin_selection) the logits are
        rewritten IN PLACE first.  A missing kernel is an error, not a fallback."""
        c = self.sel
        T, k, p = c.params
        if c.process:
            theta, ngram, min_new, min_len = c.processors
            if logits.dtype != torch.float16 or runtime.process_logits_f16(
                    logits, c.tokens, c.col0, c.step, repetition_penalty=theta, no_repeat_ngram_size=ngram, min_new_tokens=min_new,
                    min_length=min_len, eos=c.eos, scratch=c.scratch) is None:
                raise ValueError("DecodeSession.select: pbl_process_logits_f16 declines these logits (runtime.process_logits_ok)")
        if runtime.select_token_f16(logits, c.step, c.unfinished, c.tokens, c.col0, self.static_ids, c.count, c.status,
                                    temperature=T, top_k=k, top_p=p, uniforms=c.uniforms, eos=c.eos, pad=c.pad, min_p=c.min_p) is None:
            raise ValueError("DecodeSession.select: pbl_select_token_minp_f16 declines these logits (runtime.select_token_ok)")

    def _unit(self):
        self.select(self._forward(self.static_ids))

    @torch.no_grad()
    def step_select(self) -> None:
        """one decode step over the tokens the last selection left in static_ids, and the selection of the next ones: with
        graph=True ONE replay of a unit captured on the first call"""
        self._advance(1)
        if not self.use_graph:
            return self._unit()
        if self.sel_graph is None:
            c = self.sel
            self.sel_graph, _ = self._capture(self._unit, [self.static_ids, c.step, c.unfinished, c.count, c.status, c.tokens])
        self.sel_graph.replay()

    @torch.no_grad()
    def run_selection(self, n: int, poll_every: int = 8) -> int:
        """up to n more step_select calls; with eos ids, the device's count of unfinished rows is read after every poll_every-th new
        token of the generation and the loop ends once it is zero (rows that had finished receive pad meanwhile).  Returns the
        number of new tokens generated so far (the first one comes from select on the prefill's logits)."""
        c = self.sel
        for _ in range(n):
            if c.eos is not None and c.done % poll_every == 0 and int(c.count) == 0:
                break
            self.step_select()
            c.done += 1
        return c.done

    def selection_result(self) -> torch.Tensor:
        """the prompt and the new tokens so far, cut after the column at which the last row finished (what a check after every
        token would have returned); RuntimeError if a sampled row held NaN or +inf (torch.multinomial raises for such a row)"""
        c = self.sel
        status = int(c.status)
        if status & 1:
            raise RuntimeError("generate: a row of logits held NaN or +inf (or nothing finite) while sampling")
        if status & 2:
            raise RuntimeError("generate: the selection step ran outside the result buffer or the table of uniforms")
        P, done = c.col0, c.done
        if c.eos is not None and done:
            hit = torch.isin(c.tokens[:, P:P + done], c.eos)
            first = torch.where(hit.any(1), hit.int().argmax(1) + 1, done)
            done = int(first.max())
        return c.tokens[:, :P + done]

    # ---- prompt-lookup speculative decoding (greedy) on the device
    @torch.no_grad()
    def begin_speculation(self, prompt: torch.Tensor, total: int, draft_tokens: int = 3, max_ngram: int = 2, eos=(),
                          pad: int | None = None, logits: torch.Tensor | None = None) -> torch.Tensor:
        """Start a greedy generation that verifies draft_tokens = K drafted tokens per step (batch * (1 + K) <= 4 rows: one decode
        launch): prefills `prompt` [batch, P < total] (unless `logits` are the logits of a prefill the caller has just run), chooses
        the first token, drafts the first K from n-grams of at most max_ngram (1 .. 4) tokens of the row's own history, and returns the
        result `tokens` [batch, total].  The session must hold K positions of slack: max_length >= total - 1 + K (a step appends
        1 + K cache rows before the rejected ones are taken back).  eos / pad as in begin_selection."""
        K, dev = int(draft_tokens), self.device
        if prompt.dim() != 2 or prompt.shape[0] != self.batch or not prompt.shape[1] < total:
            raise ValueError(f"DecodeSession.begin_speculation: prompt must be [{self.batch}, P < total]")
        if K < 0 or not 1 <= max_ngram <= runtime.SPEC_MAX_NGRAM:
            raise ValueError("DecodeSession.begin_speculation: draft_tokens >= 0 and max_ngram in 1 .. 4")
        if self.max_length < total - 1 + K:
            raise ValueError(f"DecodeSession.begin_speculation: max_length = {self.max_length} < total - 1 + draft_tokens = {total - 1 + K}")
        if logits is None:
            logits = self.prefill(prompt)
        if logits.dtype != torch.float16 or not runtime.spec_verify_ok(self.batch, 1 + K, logits.shape[-1]):
            raise ValueError("DecodeSession.begin_speculation: pbl_spec_verify_f16 declines these logits (runtime.spec_verify_ok)")
        P = int(prompt.shape[1])
        tokens = torch.zeros(self.batch, total, dtype=torch.long, device=dev)
        tokens[:, :P] = prompt
        eos = [int(e) for e in eos]
        state = torch.tensor([P, self.batch], dtype=torch.long, device=dev)
        c = self.spec = _Speculation(
            tokens=tokens, col0=P, total=int(total), K=K, max_ngram=int(max_ngram), pad=0 if pad is None else int(pad),
            eos=torch.tensor(eos, dtype=torch.long, device=dev) if eos else None,
            ids=torch.zeros(self.batch, 1 + K, dtype=torch.long, device=dev), state=state, cursor=state[:1],
            count=state[1:].view(torch.int32)[:1], unfinished=torch.ones(self.batch, dtype=torch.bool, device=dev),
            status=torch.zeros(1, dtype=torch.int32, device=dev), stats=torch.zeros(8, dtype=torch.long, device=dev),
            positions=torch.tensor([lay.cumulative_length.data_ptr() for lay in self.cache.layers], dtype=torch.long, device=dev))
        self.spec_graph = None                                 # a captured unit holds the previous speculation's tensors
        first = torch.zeros(self.batch, dtype=torch.long, device=dev)
        if runtime.select_token_f16(logits, torch.zeros(1, dtype=torch.long, device=dev), c.unfinished, tokens, P, first, c.count,
                                    c.status, eos=c.eos, pad=c.pad) is None:
            raise ValueError("DecodeSession.begin_speculation: pbl_select_token_f16 declines these logits (runtime.select_token_ok)")
        c.ids[:, 0] = first
        c.cursor.fill_(P + 1)
        if K and runtime.ngram_draft(tokens, c.cursor, c.unfinished, c.ids, c.max_ngram) is None:
            raise ValueError("DecodeSession.begin_speculation: pbl_ngram_draft declines this shape")
        return tokens

    def _spec_unit(self):
        c = self.spec
        S = 1 + c.K
        out = self.model(c.ids, attention_mask=self._mask(S), past_key_values=self.cache, use_cache=True, logits_to_keep=S)
        if runtime.spec_verify_f16(out.logits[:, -S:], c.ids, c.tokens, c.cursor, c.unfinished, c.count, c.status, c.positions, c.stats,
                                   eos=c.eos, pad=c.pad, max_ngram=c.max_ngram if c.K else 0) is None:
            raise ValueError("DecodeSession.step_speculate: pbl_spec_verify_f16 declines these logits (runtime.spec_verify_ok)")

    def _poll(self) -> tuple[int, int]:
        """(cursor, unfinished rows): the one device read of the speculation loop; the host's position count becomes the truth"""
        c = self.spec
        cur, live = c.state.tolist()
        c.polls += 1
        self.pos = cur - 1                                     # every emitted token but the last is in the cache
        return cur, live

    @torch.no_grad()
    def step_speculate(self, drafts: torch.Tensor | None = None) -> None:
        """one speculative step over the last token and the K drafts in the unit's input: with graph=True ONE replay of a unit
        captured on the first call.  drafts [batch, K]: the caller's drafts replace the n-gram ones for this step (another drafter).
        Between polls the host counts 1 + K positions per step; before that count would refuse a step it reads the true one."""
        c = self.spec
        if drafts is not None:
            if tuple(drafts.shape) != (self.batch, c.K):
                raise ValueError(f"DecodeSession.step_speculate: drafts must be [{self.batch}, {c.K}]")
            c.ids[:, 1:].copy_(drafts)
        if self.pos + 1 + c.K > self.max_length:
            self._poll()
        self._advance(1 + c.K)
        if not self.use_graph:
            return self._spec_unit()
        if self.spec_graph is None:
            self.spec_graph, _ = self._capture(self._spec_unit, [c.ids, c.state, c.unfinished, c.status, c.stats, c.tokens])
        self.spec_graph.replay()

    @torch.no_grad()
    def run_speculation(self, poll_every: int = 8) -> int:
        """speculative steps until the result is full or every row has finished.  The host reads [cursor, unfinished rows] once per
        poll; the next poll comes after as many steps as the remaining tokens need at full acceptance, ceil(remaining / (1 + K)) -- no
        step runs after the last token -- and, with eos ids, after at most poll_every steps (steps after every row finished emit
        nothing: the result does not depend on poll_every).  Returns the number of new tokens."""
        c = self.spec
        if poll_every < 1:
            raise ValueError("DecodeSession.run_speculation: poll_every must be >= 1")
        while True:
            cur, live = self._poll()
            if cur >= c.total or live == 0:
                return cur - c.col0
            need = -(-(c.total - cur) // (1 + c.K))
            for _ in range(need if c.eos is None else min(poll_every, need)):
                self.step_speculate()

    def speculation_result(self) -> torch.Tensor:
        """the prompt and the new tokens so far, cut after the column at which the last row finished (selection_result's rule)"""
        c = self.spec
        cur, _ = self._poll()
        if int(c.status) & 2:
            raise RuntimeError("generate: the speculation step ran outside the result buffer")
        P, done = c.col0, cur - c.col0
        if c.eos is not None and done:
            hit = torch.isin(c.tokens[:, P:P + done], c.eos)
            first = torch.where(hit.any(1), hit.int().argmax(1) + 1, done)
            done = int(first.max())
        return c.tokens[:, :P + done]

    def speculation_stats(self) -> dict:
        """steps run, drafts accepted and new tokens (the first one included): tokens == 1 + steps + accepted"""
        steps, accepted, emitted = self.spec.stats[:3].tolist()
        return dict(steps=steps, accepted=accepted, tokens=1 + emitted)

    def reset(self):
        """zero the cache rows and positions (the captured step stays valid: same tensors)"""
        self.cache.reset()
        self.pos = 0


def _generation_limits(model: nn.Module, prompt_len: int, max_length=None, max_new_tokens=None, eos_token_id=None,
                       pad_token_id=None) -> tuple[int, list, int | None]:
    """(total length, eos ids, pad id) as model.generate resolves them for greedy decoding: max_new_tokens wins over max_length;
    without either, the generation config's max_new_tokens, else its max_length NEW tokens (capped at max_position_embeddings);
    ValueError where nothing is left to generate.  eos defaults to the generation config's, pad to its pad_token_id, else the
    first eos id"""
    gc = getattr(model, "generation_config", None)
    if max_new_tokens is None and max_length is None:
        max_new_tokens = getattr(gc, "max_new_tokens", None)
    if max_new_tokens is not None:
        if int(max_new_tokens) < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        total = prompt_len + int(max_new_tokens)
    elif max_length is not None:
        total = int(max_length)
    else:                                          # the config's max_length counts NEW tokens then, within max_position_embeddings
        total = prompt_len + int(getattr(gc, "max_length", None) or 20)
        cap = getattr(getattr(model, "config", None), "max_position_embeddings", None)
        total = min(total, cap) if cap is not None else total
    if total <= prompt_len:
        raise ValueError(f"Input length of input_ids is {prompt_len}, but `max_length` is set to {total}: set max_new_tokens")
    if eos_token_id is None:
        eos_token_id = getattr(gc, "eos_token_id", None)
    eos = [] if eos_token_id is None else [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])]
    if pad_token_id is None:
        pad_token_id = getattr(gc, "pad_token_id", None)
    if pad_token_id is None and eos:
        pad_token_id = eos[0]
    return total, eos, None if pad_token_id is None else int(pad_token_id)


_GREEDY_DEFAULTS = {"do_sample": False, "num_beams": 1, "use_cache": True}
_SAMPLING_ARGS = ("temperature", "top_k", "top_p")
_PROCESSOR_ARGS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length")   # greedy and sampled; min_p: sampled
_LOOKUP_ARGS = ("prompt_lookup_num_tokens", "max_matching_ngram_size")      # greedy only: prompt-lookup speculative decoding


def _sampling_params(model: nn.Module, temperature=None, top_k=None, top_p=None) -> tuple[float, int, float]:
    """(temperature, top_k, top_p) as model.generate resolves them for do_sample=True: the argument, else the value in
    model.generation_config, else -- for fields still None -- transformers' GenerationConfig._get_default_generation_params().
    temperature 1.0, top_k 0 and top_p 1.0 mean "off" (HF builds no warper for them)."""
    from transformers import GenerationConfig
    gc = getattr(model, "generation_config", None)
    defaults = GenerationConfig._get_default_generation_params()
    vals = []
    for name, v in (("temperature", temperature), ("top_k", top_k), ("top_p", top_p)):
        v = getattr(gc, name, None) if v is None else v
        vals.append(defaults[name] if v is None else v)
    return float(vals[0]), int(vals[1]), float(vals[2])


def _processor_params(model: nn.Module, prompt_len: int, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
                      min_length=None, min_p=None) -> tuple[float, int, int, int, float]:
    """(repetition_penalty, no_repeat_ngram_size, min_new_tokens, min_length, min_p) as model.generate resolves them for a prompt
    of prompt_len tokens: the argument, else the value in model.generation_config, else transformers' default (_sampling_params'
    rule; min_new_tokens and min_p have none and stay off).  A min_new_tokens that is set replaces min_length by prompt_len +
    min_new_tokens, as _prepare_generated_length does.  1.0 / 0 / 0 / 0 / 0.0 mean "off" (HF builds no processor for them; it
    builds the two length processors only with an eos id, and the min_p warper only for do_sample=True)."""
    from transformers import GenerationConfig
    gc = getattr(model, "generation_config", None)
    defaults = GenerationConfig._get_default_generation_params()
    vals = {}
    for name, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size),
                    ("min_new_tokens", min_new_tokens), ("min_length", min_length), ("min_p", min_p)):
        v = getattr(gc, name, None) if v is None else v
        vals[name] = defaults.get(name) if v is None else v
    if vals["min_new_tokens"] is not None:
        vals["min_length"] = int(vals["min_new_tokens"]) + prompt_len
    return (float(vals["repetition_penalty"]), int(vals["no_repeat_ngram_size"]), int(vals["min_new_tokens"] or 0),
            int(vals["min_length"] or 0), float(vals["min_p"] or 0.0))


@torch.no_grad()
def generate(model: nn.Module, input_ids: torch.Tensor, max_length: int | None = None, max_new_tokens: int | None = None,
             eos_token_id=None, pad_token_id: int | None = None, attention_mask: torch.Tensor | None = None, graph: bool = True,
             generator: torch.Generator | None = None, uniforms: torch.Tensor | None = None, poll_every: int = 8,
             kv_cache: str = "fp16", **kwargs) -> torch.Tensor:
    """Decoding of an unpadded batch input_ids [B, P] on the GPU: greedy -- what model.generate(input_ids, do_sample=False, ...)
    returns -- or, with do_sample=True, sampling with temperature / top_k / top_p / min_p (values not passed are resolved as
    model.generate resolves them: _sampling_params, _processor_params).  repetition_penalty, no_repeat_ngram_size (at most 8) and
    min_new_tokens / min_length act in both modes, on the device too (pbl_process_logits_f16 in front of the selection, inside the
    captured unit; HF's fp32 result rounded to fp16) -- also when only the model's generation_config sets them.  The result is the
    prompt followed by the new tokens, rows that met eos padded with pad_token_id, ending where every row has finished or at the
    length limit.  One DecodeSession: the prompt is prefilled eagerly, then each token replays ONE captured unit -- the decode step
    and the HIP token selection (pbl_select_token_minp_f16), which writes the token into the result and into the next step's input
    and keeps the eos / pad bookkeeping on the device.  The host reads the count of unfinished rows every `poll_every` tokens (never
    without an eos id); tokens generated after every row finished are pad and are cut off, so the result does not depend on
    poll_every.

    Sampling draws its uniforms ONCE per call, before the loop: torch.rand([new tokens, B]) from `generator` (default: the default
    generator of the model's device, so torch.manual_seed(n) reproduces a run), or the caller's table `uniforms` [>= new tokens, B]
    (values in [0, 1)).  graph=True and graph=False consume the same numbers and give the same tokens.  The token stream for a
    given seed differs from model.generate's (torch.multinomial consumes the generator differently); the distribution is the same,
    up to HF's arbitrary choice inside a block of tied values at the top-p boundary.

    Handed to model.generate unchanged: an attention_mask with zeros (a padded batch), a model off the GPU, beams, any other
    generation argument (typical_p, bad_words_ids, ...), do_sample=False together with sampling arguments (min_p among them),
    sampling or logits processors on a model whose logits are not fp16, no_repeat_ngram_size > 8, values HF itself refuses (it
    raises), and logits processors together with prompt_lookup_num_tokens (the verify kernel takes the raw arg-max).  A minimum
    length without an eos id processes nothing (HF builds no processor) and hands nothing over.  model.generate cannot honour
    `generator` or `uniforms`, so a call that passes one of them and must be handed over raises ValueError.  Greedy decoding of
    logits that are not fp16 keeps the selection in torch.

    prompt_lookup_num_tokens (with max_matching_ngram_size, default 2, at most 4 here), greedy decoding only: prompt-lookup speculative
    decoding on the device (DecodeSession.begin_speculation / run_speculation).  Each step feeds the last token and K =
    min(prompt_lookup_num_tokens, 4 // B - 1) tokens drafted from the row's own history, and keeps the drafts that the greedy choice
    confirms plus one more token: the greedy tokens, up to the effect of fp16 rounding on near-ties (a step of 1 + K rows and a step
    of one row round differently).  K < 1, logits that are not fp16, a shape the entries decline or K slack positions that would pass
    max_position_embeddings: the one-token loop above.  With do_sample=True the call is handed to model.generate.

    kv_cache="fp8": the session's cache rows are FP8 (DecodeSession(..., kv_cache="fp8"), which states what the model must be); the
    argument is not forwarded to model.generate, which has no such cache, so a call that must be handed over raises ValueError."""
    if kv_cache not in KV_CACHE_FORMATS:
        raise ValueError(f"generate: kv_cache must be one of {KV_CACHE_FORMATS}, not {kv_cache!r}")
    sample = kwargs.get("do_sample", False) is True
    fixed = {k: v for k, v in _GREEDY_DEFAULTS.items() if not (sample and k == "do_sample")}
    known = set(_GREEDY_DEFAULTS) | set(_SAMPLING_ARGS + ("min_p",) if sample else _LOOKUP_ARGS) | set(_PROCESSOR_ARGS)
    native = all(kwargs[k] == v for k, v in fixed.items() if k in kwargs) and not set(kwargs) - known
    padded = attention_mask is not None and not bool(attention_mask.all())
    T, top_k, top_p = 1.0, 0, 1.0                          # greedy: everything off
    if native and sample:
        T, top_k, top_p = _sampling_params(model, *(kwargs.get(k) for k in _SAMPLING_ARGS))
        native = T > 0 and top_k >= 0 and 0 < top_p <= 1 and model.get_input_embeddings().weight.dtype == torch.float16
    theta, no_repeat, min_new, min_len, min_p = 1.0, 0, 0, 0, 0.0
    if native and input_ids.dim() == 2:
        theta, no_repeat, min_new, min_len, min_p = _processor_params(
            model, input_ids.shape[1], *(kwargs.get(k) for k in _PROCESSOR_ARGS), kwargs.get("min_p") if sample else None)
        if not sample:
            min_p = 0.0                                        # HF builds warpers for do_sample=True only
        if not (theta > 0 and 0 <= no_repeat <= runtime.PROCESS_MAX_NGRAM and 0 <= min_p <= 1):
            native = False                                     # HF's own errors, or an n-gram size beyond the kernel's

    def hand_over():
        if kv_cache != "fp16":
            raise ValueError(f"generate: kv_cache={kv_cache!r} belongs to the decode loop on the GPU (an unpadded batch on a GPU model, "
                             "greedy or temperature / top_k / top_p / min_p sampling); model.generate cannot honour it")
        if generator is not None or uniforms is not None:
            raise ValueError("generate: generator= and uniforms= belong to the sampling loop on the GPU (an unpadded batch on a GPU model "
                             "with fp16 logits, do_sample=True with temperature / top_k / top_p / min_p and the logits processors "
                             "of _processor_params only); model.generate cannot honour them")
        hf = dict(kwargs)
        for k, v in (("max_length", max_length), ("max_new_tokens", max_new_tokens), ("eos_token_id", eos_token_id),
                     ("pad_token_id", pad_token_id), ("attention_mask", attention_mask)):
            if v is not None:
                hf[k] = v
        return model.generate(input_ids, **hf)

    if not native or padded or not input_ids.is_cuda or input_ids.dim() != 2:
        return hand_over()
    if poll_every < 1:
        raise ValueError("generate: poll_every must be >= 1")
    B, P = input_ids.shape
    total, eos, pad = _generation_limits(model, P, max_length, max_new_tokens, eos_token_id, pad_token_id)
    # whether a step would process anything -- begin_selection's rule: HF builds the two length processors only with an eos id
    processing = theta != 1.0 or no_repeat > 0 or (bool(eos) and (min_new > 0 or min_len > P))
    if processing and (kwargs.get("prompt_lookup_num_tokens") is not None or model.get_input_embeddings().weight.dtype != torch.float16):
        return hand_over()                                 # the verify kernel takes the raw arg-max; the kernel takes fp16 logits
    K = 0
    if kwargs.get("prompt_lookup_num_tokens") is not None:
        lookup, ngram = int(kwargs["prompt_lookup_num_tokens"]), int(kwargs.get("max_matching_ngram_size") or 2)
        if lookup < 1 or ngram < 1:
            raise ValueError("generate: prompt_lookup_num_tokens and max_matching_ngram_size must be >= 1")
        K = max(0, min(lookup, runtime.SPEC_MAX_ROWS // B - 1))
        cap = getattr(getattr(model, "config", None), "max_position_embeddings", None)
        if model.get_input_embeddings().weight.dtype != torch.float16 or (cap is not None and total - 1 + K > cap):
            K = 0
    sess = DecodeSession(model, B, total - 1 + K, graph=graph, **({} if kv_cache == "fp16" else {"kv_cache": kv_cache}))
    logits = sess.prefill(input_ids)
    if K and logits.dtype == torch.float16 and runtime.spec_verify_ok(B, 1 + K, logits.shape[1]):
        sess.begin_speculation(input_ids, total, draft_tokens=K, max_ngram=min(ngram, runtime.SPEC_MAX_NGRAM), eos=eos, pad=pad, logits=logits)
        sess.run_speculation(poll_every)
        return sess.speculation_result()
    if logits.dtype == torch.float16 and runtime.select_token_ok(B, logits.shape[1]):
        table = None
        if sample:
            if uniforms is not None:
                table = uniforms
            else:                                          # one draw for the whole call; a host generator draws on the host
                gdev = generator.device if generator is not None else input_ids.device
                table = torch.rand(total - P, B, generator=generator, device=gdev, dtype=torch.float32)
        sess.begin_selection(input_ids, total, eos=eos, pad=pad, uniforms=table, temperature=T, top_k=top_k, top_p=top_p,
                             repetition_penalty=theta, no_repeat_ngram_size=no_repeat, min_new_tokens=min_new, min_length=min_len,
                             min_p=min_p)
        sess.select(logits)
        sess.sel.done = 1
        sess.run_selection(total - P - 1, poll_every)
        return sess.selection_result()
    if sample or processing:
        return hand_over()
    out = [input_ids]
    eos_t = torch.tensor(eos, dtype=input_ids.dtype, device=input_ids.device) if eos else None
    unfinished = torch.ones(B, dtype=torch.bool, device=input_ids.device)
    cur = P
    while True:
        nxt = logits.float().argmax(-1).to(input_ids.dtype)
        if eos_t is not None:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            unfinished &= ~torch.isin(nxt, eos_t)
        out.append(nxt[:, None])
        cur += 1
        if cur >= total or (eos_t is not None and not bool(unfinished.any())):
            break
        logits = sess.step(nxt)
    return torch.cat(out, 1)
