"""What the frozen backbones (``mmfusion.vit.NativeViT``, ``mmfusion.wav2vec2.NativeWav2Vec2`` and its subclass
``mmfusion.wavlm.NativeWavLM``, ``mmfusion.deberta.NativeDeberta``, ``mmfusion.bert.NativeBert`` / ``NativeRoberta``,
``mmfusion.whisper.NativeWhisperEncoder``) share: the table of frozen parameters behind HuggingFace's ``state_dict`` surface, the chunk workspace, what is derived from
the weights once per weight version, and the launches of a transformer layer.

A layer is two blocks on ``rows = n * T`` tokens of a chunk of ``n`` items (bf16 residual stream like MulT's).  Where the
LayerNorms go around them is ``_post_ln_layer`` (Wav2Vec2's base family, DeBERTa) or ``_pre_ln_layer`` (ViT, Wav2Vec2's layer-norm family):

    _attention(src, resid, attend):
      fused Q/K/V linear + bias     mmf_gemm_grouped NT, BIAS            src -> qkv (rows, 3 d)
      attend(qkv, att)              mmf_attn_fwd_grouped by default      qkv -> att   (H heads of 64 / 96; a subclass hands in
                                                                                       its own attention: DeBERTa's disentangled one)
      out-projection + bias + resid mmf_gemm_grouped NT, BIAS | ADD_AUX  att -> y
    _ffn(src, resid, out):
      fc1                           mmf_gemm_grouped NT                  src -> h (rows, intermediate)
      + bias, exact GELU            mmf_bias_gelu_bf16 (in place)        h
      fc2 + bias + resid            mmf_gemm_grouped NT, BIAS | ADD_AUX  h   -> out
    (both blocks end in ``_closing``: with a model's ``join`` hook the closing launch is BIAS only and ``join(role, y, resid)`` makes
     the sum; training-mode hidden dropout, ``_hidden_joins``.  Without one, the rows above.)
    _ln(src, dst)                   mmf_layernorm_fwd_grouped            src -> dst
    _widen(src, dst)                mmf_cast_bf16_to_f32                 src -> the f32 result
    _ln_bwd(...)                    mmf_layernorm_bwd_grouped            dy  -> dx (the input gradient; the backbones' backward)
    _ln_bwd(..., resid=r)           mmf_layernorm_bwd_add_grouped        dy, r -> dx = r + that (a pre-LN layer's residual gradient)
    _wgrad(dy, x, name, slabs)      mmf_gemm_grouped TN, COLSUM_A        dy, x -> a trainable layer's weight and bias gradients; in
                                    (+ mmf_sum_slabs_f32)                ``slabs`` K-slabs where the output is a few tiles under many rows

The backward of a post-LN layer is ``_post_ln_layer_grad`` (Wav2Vec2's base family, DeBERTa; a pre-LN layer's is
``_pre_ln_layer_grad``, which ViT and Wav2Vec2's layer-norm family share; ViT's CLS form is its own ``_layer_grad``): the layer
again from its saved input ``xin``, then top down, on the backward's workspace (``_grad_workspace``;
``ga`` holds the gradient of the layer's output on entry and of ``xin`` on return)

      _attention(xin, + xin, attend)                                           xin -> qkv -> att -> y1 (the attention writes lse)
      LayerNorm 1                   mmf_layernorm_fwd_grouped                  y1  -> ln   (mean1, rstd1)
      fc1; + bias, GELU beside it   NT; mmf_bias_gelu_bf16_to                  ln  -> h (raw) -> g
      fc2 + bias + ln               NT, BIAS | ADD_AUX                         g   -> y2
      LayerNorm 2                   mmf_layernorm_fwd_grouped                  y2  -> (mean2, rstd2; the output is not read)
      LayerNorm 2 backward          mmf_layernorm_bwd_grouped                  ga  -> gb = dy2
      fc2 wgrad, dgrad              mmf_gemm_grouped TN (COLSUM_A) / NN        gb  -> dh = dg
      GELU backward                 mmf_bias_gelu_bwd_bf16 (in place)          dh, h -> dh
      fc1 wgrad, dgrad + dy2        TN / NN, ADD_AUX                           dh  -> ga = dln1
      LayerNorm 1 backward          mmf_layernorm_bwd_grouped                  ga  -> gb = dy1
      out-projection wgrad, dgrad   TN / NN                                    gb  -> ga = datt
      attn_bwd(qkv, att, datt, dqkv)                                           ga  -> dqkv
      qkv_wgrad(dqkv, xin)          TN                                         the fused Q/K/V weight and bias gradients
      Q/K/V dgrad + dy1             NN, ADD_AUX                                dqkv -> ga = dxin (``below`` only)

A model supplies four things: the attention forward, the attention backward, the Q/K/V weight gradient (None: the frozen walk,
which forms no weight gradient at all and discards the LayerNorms' parameter sums) and the K-slab rule of the other weight
gradients (None: plain launches).

Parameters are stored as the kernels read them (Q/K/V fused, a subclass may store a weight with its last two dims swapped)
and ``_hf`` maps every HuggingFace key to its view of them, in HuggingFace's order, so ``state_dict()`` and
``load_state_dict`` speak HuggingFace's names and shapes; ``_add_layer`` registers one layer from a table of HuggingFace's
names.  A subclass declares its workspace as a table of (name, elements per chunk item, dtype), ``_ws_table(size)``, and its
backward's as ``_grad_table(size)``; the allocation and the bytes-per-item figure are both read from that table.  A forward pass writes no attribute of the module
but that workspace and the ``_derived`` cache: what a launch needs beyond the buffers travels as arguments.

Frozen by default: every parameter has ``requires_grad = False`` and the outputs carry no autograd graph.  Every backbone has a
backward: ``NativeDeberta`` called with input embeddings that require a gradient (prompt tuning), and all three with their top
layers marked trainable (``set_trainable_layers``: those layers' parameters then require a gradient and a call in grad mode adds
their gradients into the parameter arena), mmfusion/deberta.py, mmfusion/vit.py and mmfusion/wav2vec2.py.  bf16
storage only: in the fp32 parity mode (``ops.fp32_mode()``) the forward raises instead of computing something else.
Nothing synchronises with the host: a fixed-shape call can be captured by ``torch.cuda.graph``.

Training-mode dropout (DeBERTa's dropout, Wav2Vec2's regularisers; each model's docstring has its table of sites).  A differentiable
call in ``train()`` mode with a probability above 0 owns one ``_CallDropout``: it takes its sites from ``ops.next_site()`` in
HuggingFace's call order, a model's leading sites and then four per layer, and keeps them for its backward.  Every mask is the counter
hash of (``ops.rng_state()``, site, sub-stream, index) with sub-stream = the item's index in the WHOLE batch (attention: that times
H plus the head) and index = the element's place within the item, never a function of the launch: a chunk that starts at item
``n0`` passes ``n0`` as ``item0`` and draws what the whole batch would, so no result depends on ``chunk``.  Nothing is stored: the
state is read where a launch is made (live, as ``ops._Dropout.backward`` does), the recomputed layer regenerates its masks and the
backward's own kernels draw them again from the same (state, site, item0).  The hidden sites of a layer are ``_closing``'s ``join``
hook (``_hidden_joins``: the closing launch is BIAS only, ``mmf_hidden_dropout`` forms bf16(fma(dense + bias, keep c, resid)); the
gradient of a pre-LN sum reaches the dense branch through the same kernel and the residual branch as it is).  A call on its own (no
root module's forward around it) starts a training forward itself, so successive calls draw new masks (``_own_training_forward``).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import arena as _arena
from . import lib, ops
from .lib import EPI_ACCUM, EPI_ADD_AUX, EPI_BIAS, EPI_COLSUM_A, GEMM_NN, GEMM_NT, GEMM_TN, AttnProblem, LnProblem

BF16 = torch.bfloat16
LN_WIDTHS = (256, 512, 768, 1024)          # the lane forms of layernorm.hip
LN_MAX_WIDTH = 2048                        # its chunk form: every multiple of 8 up to this (forward; a frozen model needs no more)
WsTable = List[Tuple[str, int, torch.dtype]]
Attend = Callable[[torch.Tensor, torch.Tensor], None]          # (qkv rows, att rows): launches one chunk's attention
AttnBwd = Callable[[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor], None]     # (qkv, att, datt, dqkv rows): its backward
QkvWgrad = Callable[[torch.Tensor, torch.Tensor], None]        # (dqkv rows, the projection's input rows): the fused weight's gradient
# What stands between a block's closing dense launch and its LayerNorm where a model has something there (training-mode hidden
# dropout; absent: the residual add is the GEMM's epilogue).  Join(role, y, resid): role "o" / "fc2", y = dense + bias as bf16 -> the
# pre-LN sum, in place.  JoinBwd(role, dy, out): the gradient dy of that sum -> out, the dense branch's share of it
Join = Callable[[str, torch.Tensor, torch.Tensor], None]
JoinBwd = Callable[[str, torch.Tensor, torch.Tensor], None]
# A model's own activation launches, (forward(h, bias, g), backward(dg, h, bias, dh)) with ``lib.bias_gelu_to`` / ``bias_gelu_bwd``'s
# arguments (Wav2Vec2's training-mode activation dropout; absent: those two)
Act = Tuple[Callable[[torch.Tensor, torch.Tensor, torch.Tensor], None], Callable[[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor], None]]


def _check_probability(who: str, name: str, p, closed: bool = False) -> None:
    """``p`` must be a number (no bool) in [0, 1), with ``closed`` in [0, 1]; the error names the call as ``who(name=p)``"""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= p <= 1.0 if closed else 0.0 <= p < 1.0):
        raise ValueError(f"{who}({name}={p!r}): a probability in [0, 1{']' if closed else ')'}")


class _CallDropout:
    """The dropout of one differentiable training call (the module docstring has the keying): the hidden and the attention
    probability and the call's sites, ``lead`` leading ones and then four per layer, taken from ``ops.next_site()`` in that order.  A
    model's subclass names them in HuggingFace's call order and adds what else its call keeps."""

    def __init__(self, p_h: float, p_a: float, lead: int, layers: int):
        self.p_h, self.p_a = p_h, p_a
        self.lead = tuple(ops.next_site() for _ in range(lead))
        self.layers = [tuple(ops.next_site() for _ in range(4)) for _ in range(layers)]

    @staticmethod
    def key(p: float, site: int, item0: int) -> tuple:
        """what a launch with keyed dropout takes (``lib._drop_args``); the state is read here, live: the backward draws the
        forward's masks from the same state"""
        return p, ops.rng_state(), site, item0

    def hidden(self, site: int, item0: int) -> tuple:
        return self.key(self.p_h, site, item0)

    def join_sites(self, i: int) -> Tuple[int, int]:
        """layer ``i``'s hidden sites behind its two closing launches (``FrozenBackbone._hidden_joins``); ``OUT`` / ``MLP``: the
        subclass's places of them among the layer's four"""
        return self.layers[i][self.OUT], self.layers[i][self.MLP]


class BackboneOutput:
    """What the encoders read from a backbone's result."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = None


class FrozenBackbone(nn.Module):
    """Base of the native backbones.  A subclass declares its limits to ``__init__`` (``head_dims``: the head widths its
    attention has a form for; ``ln_widths``: further named sizes that go through the LayerNorm kernel; ``ln_any_width``: the model
    runs the LayerNorm forward only, whose chunk form takes every multiple of 8 up to 2048 where no lane form does), sets ``self.config``
    (``hidden_size``, ``num_attention_heads``, ``intermediate_size``, ``layer_norm_eps``), registers its parameters with ``_add``
    / ``_add_layer`` in HuggingFace's order, and defines ``_ws_table(size)``."""

    def __init__(self, hidden_size: int, num_attention_heads: int, chunk: int, head_dims: Sequence[int] = (64, 96),
                 ln_widths: Optional[Dict[str, int]] = None, ln_any_width: bool = False):
        super().__init__()
        d, H, who = hidden_size, num_attention_heads, type(self).__name__
        if H <= 0 or d % H or d // H not in head_dims:
            raise ValueError(f"{who}: hidden_size {d} / num_attention_heads {H} must give a head_dim of "
                             f"{' or '.join(str(v) for v in head_dims)} (its attention kernel's forms)")
        for name, width in {"hidden_size": d, **(ln_widths or {})}.items():
            if ln_any_width and (width <= 0 or width % 8 or width > LN_MAX_WIDTH):
                raise ValueError(f"{who}: {name} {width} is not a multiple of 8 up to {LN_MAX_WIDTH} (the LayerNorm forward's chunk form)")
            if not ln_any_width and width not in LN_WIDTHS:
                raise ValueError(f"{who}: {name} {width} is not one of the LayerNorm kernel's widths {LN_WIDTHS}")
        self.chunk = int(chunk)
        self.head_dim = d // H
        # HuggingFace key -> (parameter, row range | None, stored with the last two dims swapped)
        self._hf: Dict[str, Tuple[str, Optional[Tuple[int, int]], bool]] = {}
        self._ws: Optional[dict] = None
        self._cache: Dict[str, tuple] = {}             # _derived: slot -> (stamp of the parameters it was built from, value)
        self._trainable = 0                            # a subclass's set_trainable_layers
        self._gws: Optional[dict] = None               # a backward's workspace (the subclass's _grad_table), from the first differentiable call
        self._slabs: Optional[torch.Tensor] = None     # _slab_buffer

    # -- training-mode dropout ---------------------------------------------------------------------------
    @staticmethod
    def _own_training_forward() -> None:
        """A differentiable training call that is about to take its sites: on its own it starts a training forward itself (new
        masks, sites from 1); under a root module's forward it continues that forward's site numbering"""
        if not ops.inside_root():
            ops.begin_training_forward()

    @staticmethod
    def _hidden_joins(drop: Optional[_CallDropout], sites: Tuple[int, int], n: int, n0: int) -> tuple:
        """(join, join_bwd) of a layer on a chunk of ``n`` items from item ``n0`` (``Join`` / ``JoinBwd`` above): hidden dropout at
        ``sites`` = (the attention output's, the MLP output's), fused with the residual add, and its gradient form; (None, None)
        without hidden dropout"""
        if drop is None or drop.p_h <= 0.0:
            return None, None
        site = dict(zip(("o", "fc2"), sites))

        def join(role: str, y: torch.Tensor, resid: torch.Tensor) -> None:
            lib.hidden_dropout(y, y, n, drop.hidden(site[role], n0), resid=resid)

        def join_bwd(role: str, dy: torch.Tensor, out: torch.Tensor) -> None:
            lib.hidden_dropout(dy, out, n, drop.hidden(site[role], n0))
        return join, join_bwd

    # -- fine-tuning the top layers ----------------------------------------------------------------------
    @staticmethod
    def _layer_params(i: int) -> list:
        return [f"l{i}_{r}_{s}" for r in ("qkv", "o", "ln1", "fc1", "fc2", "ln2") for s in "wb"]

    @property
    def trainable_layers(self) -> int:
        return self._trainable

    def _check_trainable(self, k, flag: str, on, what: str, why: str) -> None:
        """``set_trainable_layers(k, flag=on)``'s arguments: ``k`` in 0 .. L, and the model's extras (``what``: "the embeddings
        train") with every layer only, since ``why``"""
        who, L = type(self).__name__, self.config.num_hidden_layers
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= L:
            raise ValueError(f"{who}: set_trainable_layers({k!r}): an integer in 0 .. {L} (num_hidden_layers)")
        if not isinstance(on, bool) or (on and k != L):
            raise ValueError(f"{who}: set_trainable_layers({k!r}, {flag}={on!r}): {what} with all {L} layers only ({why})")

    def _require_grad(self, names) -> None:
        """``requires_grad`` for the parameters ``names`` and for no other"""
        names = set(names)
        for name, p in self.named_parameters(recurse=False):
            p.requires_grad_(name in names)

    def _grads(self, i: int, role: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """layer ``i``'s f32 (weight, bias) gradients of ``role`` (for a LayerNorm: dgamma, dbeta)"""
        return getattr(self, f"l{i}_{role}_w").grad, getattr(self, f"l{i}_{role}_b").grad

    def _keep(self, first: int, rows: int, dev) -> torch.Tensor:
        """where a differentiable forward keeps the bf16 inputs of the layers ``first`` .. L - 1, ``rows`` rows each"""
        c = self.config
        return torch.empty((c.num_hidden_layers - first, rows, c.hidden_size), dtype=BF16, device=dev)

    # -- parameter table --------------------------------------------------------------------------------
    def _add(self, name: str, shape, key: Optional[str] = None, *, ones: bool = False, std: float = 0.02, swapped: bool = False):
        p = nn.Parameter(torch.empty(shape), requires_grad=False)
        if ones:
            nn.init.ones_(p)
        elif std > 0:
            nn.init.normal_(p, std=std)
        else:
            nn.init.zeros_(p)
        self.register_parameter(name, p)
        if key is not None:
            self._hf[key] = (name, None, swapped)

    def _add_qkv(self, i: int, d: int, keys: Dict[str, str]) -> None:
        """layer ``i``'s fused (3 d, d) projection, rows q | k | v; ``keys``: "q" / "k" / "v" -> HuggingFace's name of that
        linear, in HuggingFace's order"""
        for role, key in keys.items():
            r = "qkv".index(role)
            self._hf[key + ".weight"] = (f"l{i}_qkv_w", (r * d, r * d + d), False)
            self._hf[key + ".bias"] = (f"l{i}_qkv_b", (r * d, r * d + d), False)
        self._add(f"l{i}_qkv_w", (3 * d, d))
        self._add(f"l{i}_qkv_b", (3 * d,), std=0.0)

    def _add_layer(self, i: int, d: int, I: int, keys: Dict[str, str]) -> None:
        """layer ``i``: ``l{i}_{qkv,o,fc1,fc2}_{w,b}`` and ``l{i}_ln{1,2}_{w,b}``.  ``keys``: "q", "k", "v", "o", "ln1", "fc1",
        "fc2", "ln2" -> HuggingFace's name of that module (without ``.weight`` / ``.bias``), IN HUGGINGFACE'S ORDER for the
        model, the three projections first: that order is ``state_dict()``'s"""
        roles = list(keys)
        assert sorted(roles[:3]) == ["k", "q", "v"] and sorted(roles[3:]) == ["fc1", "fc2", "ln1", "ln2", "o"], roles
        self._add_qkv(i, d, {r: keys[r] for r in roles[:3]})
        shapes = {"o": (d, d), "fc1": (I, d), "fc2": (d, I), "ln1": (d,), "ln2": (d,)}
        for r in roles[3:]:
            self._add(f"l{i}_{r}_w", shapes[r], keys[r] + ".weight", ones=r.startswith("ln"))
            self._add(f"l{i}_{r}_b", shapes[r][:1], keys[r] + ".bias", std=0.0)

    # -- HuggingFace state_dict surface ----------------------------------------------------------------
    def _canonical_key(self, key: str) -> str:
        """a checkpoint's key in the spelling of ``_hf`` (a subclass that reads older spellings overrides this)"""
        return key

    def _view(self, name: str, rows, swapped: bool, keep_vars: bool = False) -> torch.Tensor:
        p = getattr(self, name)
        t = p if keep_vars else p.detach()
        if rows is not None:
            t = t[rows[0]:rows[1]]
        return t.permute(0, 2, 1) if swapped else t

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for key, (name, rows, swapped) in self._hf.items():
            destination[prefix + key] = self._view(name, rows, swapped, keep_vars)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        found = {}
        for key in list(state_dict.keys()):
            if not key.startswith(prefix):
                continue
            k = self._canonical_key(key[len(prefix):])
            if k in self._hf:
                found[k] = state_dict[key]
            elif strict:
                unexpected_keys.append(key)
        with torch.no_grad():
            for k, (name, rows, swapped) in self._hf.items():
                if k not in found:
                    missing_keys.append(prefix + k)
                    continue
                dst, src = self._view(name, rows, swapped), found[k]
                if tuple(src.shape) != tuple(dst.shape):
                    error_msgs.append(f"size mismatch for {prefix + k}: copying a param with shape {tuple(src.shape)} from "
                                      f"checkpoint, the shape in current model is {tuple(dst.shape)}.")
                    continue
                dst.copy_(src)                 # in place: the version counter moves, so what was derived from the old value is rebuilt

    # -- workspace --------------------------------------------------------------------------------------
    def _token_table(self, T: int, h: int) -> WsTable:
        """the layers' buffers for one item of ``T`` tokens; ``h`` elements for the MLP's hidden activations"""
        d, H = self.config.hidden_size, self.config.num_attention_heads
        return [("x", T * d, BF16), ("y", T * d, BF16), ("ln", T * d, BF16), ("att", T * d, BF16), ("qkv", T * 3 * d, BF16),
                ("h", h, BF16), ("mean", T, torch.float32), ("rstd", T, torch.float32), ("lse", H * T, torch.float32)]

    @staticmethod
    def _bytes_per_item(table: WsTable) -> int:
        return sum(numel * dtype.itemsize for _, numel, dtype in table)

    def _workspace(self, dev, size=None) -> dict:
        """the workspace of ``self.chunk`` items of ``size`` (samples, tokens; None where the model fixes it).  Every buffer
        grows with ``size``, so a smaller item uses the leading part of what a larger one allocated"""
        if not self._fits(self._ws, dev, size):
            self._ws = self._allocate(self._ws_table(size), dev, size)
        return self._ws

    def _fits(self, ws: Optional[dict], dev, size) -> bool:
        """whether the workspace ``ws`` serves ``self.chunk`` items of ``size`` on ``dev``"""
        return ws is not None and ws["dev"] == dev and ws["chunk"] == self.chunk and (size is None or ws["size"] >= size)

    def _allocate(self, table: WsTable, dev, size) -> dict:
        ws = {"dev": dev, "chunk": self.chunk, "size": size}
        for name, numel, dtype in table:
            ws[name] = torch.empty(self.chunk * numel, dtype=dtype, device=dev)
        return ws

    def _grad_rows(self, T: int, second: str = "y2") -> WsTable:
        """The layers' part of a backward's table (the subclass's ``_grad_table(size)``) for one item of ``T`` tokens, beside the
        forward workspace: ``second`` (what the layer's backward keeps of its second block: a post-LN layer's pre-LN sum ``y2``,
        ViT's ``ln2``), the GELU output ``g`` (``h`` keeps the raw fc1 output), the gradient buffers (``ga`` / ``gb`` alternate as
        the d-wide gradients, ``dh`` is dg then dh), both LayerNorms' statistics and the attention backward's delta"""
        c = self.config
        d, H, I, f32 = c.hidden_size, c.num_attention_heads, c.intermediate_size, torch.float32
        return [(second, T * d, BF16), ("g", T * I, BF16), ("ga", T * d, BF16), ("gb", T * d, BF16), ("dh", T * I, BF16),
                ("dqkv", T * 3 * d, BF16), ("mean1", T, f32), ("rstd1", T, f32), ("mean2", T, f32), ("rstd2", T, f32), ("delta", H * T, f32)]

    def _grad_scratch(self) -> Tuple[int, Dict[str, int]]:
        """what a backward holds beside its table, whatever the chunk -> (the widest LayerNorm its backward goes through: the
        width of ``dgb`` and ``ln_ws``, further f32 buffers: name -> elements).  ``junk``: where the key bias's column sum goes
        (``_qkv_wgrad_roles``; it is not kept)"""
        d = self.config.hidden_size
        return d, {"junk": d}

    def _grad_workspace(self, dev, size=None) -> dict:
        """the backward's workspace of ``self.chunk`` items of ``size``: the subclass's ``_grad_table(size)`` and
        ``_grad_scratch()``, kept and reused as ``_workspace`` is"""
        if not self._fits(self._gws, dev, size):
            width, extra = self._grad_scratch()
            f32 = lambda numel: torch.empty(numel, dtype=torch.float32, device=dev)
            g = self._allocate(self._grad_table(size), dev, size)
            g.update(dgb=f32(2 * width), ln_ws=f32(lib.load().mmf_layernorm_bwd_workspace_bytes(width) // 4), **{k: f32(v) for k, v in extra.items()})
            self._gws = g
        return self._gws

    @staticmethod
    def _stats(g: dict, k: int) -> dict:
        """the backward workspace as ``_ln`` / ``_ln_bwd`` read it for a layer's LayerNorm ``k`` (1 / 2): its statistics as
        ``mean`` / ``rstd`` beside the LayerNorm backward's scratch"""
        return {"mean": g[f"mean{k}"], "rstd": g[f"rstd{k}"], "dgb": g["dgb"], "ln_ws": g["ln_ws"]}

    def _chunks(self, N: int):
        """(first item, items) of each pass of ``N`` items through the workspace"""
        for n0 in range(0, N, self.chunk):
            yield n0, min(self.chunk, N - n0)

    @staticmethod
    def _rows(ws, name: str, rows: int, width: int) -> torch.Tensor:
        """the leading (rows, width) of a workspace buffer"""
        return ws[name][:rows * width].view(rows, width)

    # -- what is derived from the weights ---------------------------------------------------------------
    def _derived(self, slot: str, names: Sequence[str], build: Callable[[], object]):
        """``build()`` of the parameters ``names``, made once per weight version: again when one of them was written in place
        (``load_state_dict``) or replaced (``.cuda()``)"""
        stamp = tuple((p.data_ptr(), p._version) for p in (getattr(self, n) for n in names))
        hit = self._cache.get(slot)
        if hit is None or hit[0] != stamp:
            with torch.no_grad():
                hit = self._cache[slot] = (stamp, build())
        return hit[1]

    # -- launches ---------------------------------------------------------------------------------------
    def _refuse_fp32(self) -> None:
        if ops.fp32_mode():
            raise RuntimeError(f"{type(self).__name__} runs with bf16 storage only: it has no form for the fp32 parity mode (and no eager fallback)")

    def _check_input(self, x, name: str, dtype: torch.dtype = torch.float32, ndim: Optional[int] = None) -> None:
        who = type(self).__name__
        self._refuse_fp32()
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(f"{who} runs on the GPU only (no CPU fallback)")
        want = str(dtype).rpartition(".")[2]
        if ndim is not None and (x.dtype != dtype or x.dim() != ndim):
            raise TypeError(f"{who}: {name} must be {ndim}-d {want}, got {tuple(x.shape)} {x.dtype}")
        if x.dtype != dtype:
            raise TypeError(f"{who}: {name} must be {want}, got {x.dtype}")

    def _w(self, name: str) -> torch.Tensor:
        return ops.shadow(getattr(self, name))

    def _f(self, name: str) -> torch.Tensor:
        return getattr(self, name).detach()

    def _ln(self, ws, src: torch.Tensor, dst: torch.Tensor, gamma: str, beta: str) -> None:
        rows, width = src.shape
        with lib._Timed("ln_fwd_kernel", 0.0, [(rows, width)]):
            lib.layernorm_fwd_grouped([LnProblem(src.data_ptr(), dst.data_ptr(), self._f(gamma).data_ptr(), self._f(beta).data_ptr(),
                                                 ws["mean"].data_ptr(), ws["rstd"].data_ptr(), None, None, None, None, rows)],
                                      width, self.config.layer_norm_eps)

    def _ln_bwd(self, scratch, src: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, gamma: str, into=None,
                resid: Optional[torch.Tensor] = None) -> None:
        """dx = the LayerNorm input gradient of ``dy`` at the input ``src`` whose statistics are ``scratch["mean"]`` / ``["rstd"]``.
        The kernel also sums gamma / beta's gradients.  Frozen parameters (``into`` None): into ``scratch["dgb"]`` (2 width f32),
        zeroed here and discarded.  Trainable ones: ``into`` = (dgamma, dbeta), the parameters' f32 gradients, which the kernel
        adds to.  ``scratch["ln_ws"]``: its f32 workspace.  With ``resid`` (bf16 rows like dx; it may be dx) the residual gradient
        is folded in: dx = resid + the LayerNorm input gradient (a pre-LN layer: the LayerNorm's input also feeds the residual add
        behind the block, so its gradient is the sum of the two)"""
        rows, width = src.shape
        if into is None:
            dgb = scratch["dgb"]
            dgb.zero_()
            dgamma, dbeta = dgb.data_ptr(), dgb.data_ptr() + 4 * width
        else:
            dgamma, dbeta = into[0].data_ptr(), into[1].data_ptr()
        launch = lib.layernorm_bwd_grouped if resid is None else lib.layernorm_bwd_add_grouped
        with lib._Timed("ln_bwd_kernel", 0.0, [(rows, width)]):
            launch([LnProblem(src.data_ptr(), None if resid is None else resid.data_ptr(), self._f(gamma).data_ptr(), None,
                              scratch["mean"].data_ptr(), scratch["rstd"].data_ptr(), dy.data_ptr(), dx.data_ptr(), dgamma, dbeta, rows)],
                   width, scratch["ln_ws"])

    # -- weight gradients of the trainable layers ----------------------------------------------------------
    @staticmethod
    def _first_touch(wgrad: torch.Tensor) -> bool:
        """The arena's lazy-zero protocol as ``ops.queue_wgrad`` keeps it: whether the launch that is about to produce the
        gradient ``wgrad`` (a parameter's ``.grad``) must overwrite it (the first write of a step into a lazily zeroed weight
        gradient) or accumulate (every later one)"""
        ar = _arena.arena_of(wgrad)
        return ar is not None and ar.take_first_touch(wgrad)

    @staticmethod
    def _slab_bounds(rows: int, slabs: int) -> List[int]:
        """the row range [0, rows) cut into at most ``slabs`` K-slabs whose lengths are multiples of 32 (the last one takes the
        rest) and differ by at most 32 -> the slabs' first rows and ``rows``"""
        units = (rows + 31) // 32
        S = max(1, min(int(slabs), units))
        cuts, at = [0], 0
        for s in range(S):
            at += units // S + (1 if s < units % S else 0)
            cuts.append(min(rows, 32 * at))
        return cuts

    def _wgrad_launch(self, parts: Sequence[tuple], overwrite: bool, slabs: int = 1) -> None:
        """One grouped TN launch, now, in stream order (the operands are workspace views the next launch overwrites), for
        ``parts`` = (dy, x, wgrad, bgrad): wgrad (+)= dy^T x and bgrad += colsum(dy) (the GEMM's fused column sum, always added).
        ``slabs`` > 1, the K-slab form for few tiles under many rows: the parts must share their row count and their wgrads tile
        one contiguous block of a gradient in order; every part's rows are cut into ``slabs`` K-slabs (``_slab_bounds``) whose
        products land in f32 partial buffers, all in the one launch, and ``mmf_sum_slabs_f32`` writes or adds their sum, slab 0
        first, into the block.  The bias column sums go straight to bgrad in both forms"""
        if slabs <= 1:
            ops.gemm_group(GEMM_TN, [(dy, x, wg, bg, None) for dy, x, wg, bg in parts], (0 if overwrite else EPI_ACCUM) | EPI_COLSUM_A)
            return
        cuts = self._slab_bounds(parts[0][0].shape[0], slabs)
        S, total = len(cuts) - 1, sum(wg.numel() for _, _, wg, _ in parts)
        first = parts[0][2]
        block = torch.as_strided(first, (total,), (1,))
        if S > lib.SUM_SLABS_MAX or any(dy.shape[0] != cuts[-1] or not wg.is_contiguous() for dy, _, wg, _ in parts):
            raise ValueError("_wgrad_launch: the K-slab form takes parts of one row count with contiguous gradients, at most "
                             f"{lib.SUM_SLABS_MAX} slabs")
        partial = self._slab_buffer(S * total, first.device).view(S, total)
        probs, off = [], 0
        for dy, x, wg, bg in parts:
            if wg.data_ptr() != first.data_ptr() + 4 * off:
                raise ValueError("_wgrad_launch: the parts' gradients must tile one contiguous block in order")
            for s in range(S):
                probs.append((dy[cuts[s]:cuts[s + 1]], x[cuts[s]:cuts[s + 1]], partial[s, off:off + wg.numel()].view(wg.shape), bg, None))
            off += wg.numel()
        ops.gemm_group(GEMM_TN, probs, EPI_COLSUM_A)
        lib.sum_slabs(partial, block, not overwrite)

    def _slab_buffer(self, numel: int, dev) -> torch.Tensor:
        """the K-slab partial products' f32 buffer, kept beside the backward's workspace and grown on demand"""
        buf = self._slabs
        if buf is None or buf.numel() < numel or buf.device != dev:
            buf = self._slabs = torch.empty(numel, dtype=torch.float32, device=dev)
        return buf[:numel]

    def _wgrad(self, dy: torch.Tensor, x: torch.Tensor, name: str, slabs: int = 1) -> None:
        """``l{i}_{role}``'s weight gradient += dy^T x and bias gradient += colsum(dy) (``_wgrad_launch`` on the whole weight;
        ``slabs`` = 1: one plain launch)"""
        w, b = getattr(self, name + "_w").grad, getattr(self, name + "_b").grad
        self._wgrad_launch([(dy, x, w, b)], self._first_touch(w), slabs)

    @staticmethod
    def _slabs_for(rows: int, tiles: int) -> int:
        """The K-slab count of a weight-gradient launch of ``tiles`` 256 x 256 output tiles over ``rows`` rows (the host rule,
        DESIGN.md section 8): as many slabs as fill one round of the CUs with tiles, each at least 1024 rows long; 1 (the plain
        launch) where that would not reach half the CUs, below which the TN launch is the small-tile kernel's either way"""
        cus = lib.load().mmf_device_cu_count()
        cus = cus if cus > 0 else 256
        S = min(cus // tiles, rows // 1024, lib.SUM_SLABS_MAX)
        return S if S > 1 and S * tiles >= (cus + 1) // 2 else 1

    @staticmethod
    def _tiles(M: int, N: int) -> int:
        """the 256 x 256 output tiles of an (M, N) weight gradient (what ``auto_impl`` of csrc/gemm.hip counts)"""
        return ((M + 255) // 256) * ((N + 255) // 256)

    def _qkv_wgrad_roles(self, i: int, junk: torch.Tensor, dqkv: torch.Tensor, x: torch.Tensor, roles: Sequence[int] = (0, 1, 2),
                         overwrite: Optional[bool] = None) -> None:
        """The rows ``roles`` (0 / 1 / 2 = q / k / v) of layer ``i``'s fused Q/K/V weight and bias gradients from ``dqkv`` and the
        projection's input ``x``, one K-slab launch.  The key bias takes no column sum: its exact gradient is zero (a shift of
        every key by one vector moves every score of a row equally), what a column sum would add is the bf16 residue of delta and
        dK; the GEMM's column sum of that part goes to ``junk`` (hidden_size f32, not kept).  ``overwrite``: the weight's first
        touch where the caller has taken it already"""
        d = self.config.hidden_size
        w, b = self._grads(i, "qkv")
        over = self._first_touch(w) if overwrite is None else overwrite
        part = lambda r: (dqkv[:, r * d:(r + 1) * d], x, w[r * d:(r + 1) * d], junk if r == 1 else b[r * d:(r + 1) * d])
        self._wgrad_launch([part(r) for r in roles], over, self._slabs_for(x.shape[0], len(roles) * self._tiles(d, d)))

    def _attn_problem(self, ws, qkv: torch.Tensor, att: torch.Tensor, n: int, Tq: int, T: int, datt: Optional[torch.Tensor] = None,
                      delta: Optional[torch.Tensor] = None, dqkv: Optional[torch.Tensor] = None) -> AttnProblem:
        """attention of ``Tq`` queries per item over its ``T`` keys, read from the fused ``qkv`` rows; ``Tq == 1`` takes the
        query of each item's first row.  lse is the forward workspace's; the backward adds ``datt``, ``delta`` and ``dqkv``, laid
        out as ``qkv``"""
        c, d = self.config, self.config.hidden_size
        q, dq = qkv.data_ptr(), None if dqkv is None else dqkv.data_ptr()
        return AttnProblem(q, q + 2 * d, q + 4 * d, att.data_ptr(), ws["lse"].data_ptr(), None if datt is None else datt.data_ptr(),
                           None if delta is None else delta.data_ptr(), dq, dq and dq + 2 * d, dq and dq + 4 * d, n,
                           c.num_attention_heads, Tq, T, 3 * d if Tq == T else T * 3 * d, 3 * d, 3 * d, d)

    def _attn(self, ws, qkv: torch.Tensor, att: torch.Tensor, n: int, Tq: int, T: int) -> None:
        lib.attn_fwd_grouped([self._attn_problem(ws, qkv, att, n, Tq, T)], self.head_dim, self.head_dim ** -0.5)

    def _closing(self, i: int, role: str, src: torch.Tensor, resid: torch.Tensor, y: torch.Tensor, join: Optional[Join]) -> None:
        """y = resid + src W^T + b, the dense launch that closes a block (``role`` "o" / "fc2"): the residual add is its epilogue;
        with ``join`` the launch writes src W^T + b and ``join(role, y, resid)`` makes the sum of it"""
        w, b = self._w(f"l{i}_{role}_w"), self._f(f"l{i}_{role}_b")
        if join is None:
            ops.gemm(GEMM_NT, src, w, y, bias=b, aux=resid, epilogue=EPI_BIAS | EPI_ADD_AUX)
        else:
            ops.gemm(GEMM_NT, src, w, y, bias=b, epilogue=EPI_BIAS)
            join(role, y, resid)

    def _out_proj(self, i: int, att: torch.Tensor, resid: torch.Tensor, y: torch.Tensor, join: Optional[Join] = None) -> None:
        self._closing(i, "o", att, resid, y, join)

    def _attention(self, i: int, ws, src: torch.Tensor, resid: torch.Tensor, n: int, T: int, attend: Optional[Attend] = None,
                   join: Optional[Join] = None) -> torch.Tensor:
        """-> y = resid + out_proj(attention(qkv(src))) on the ``n * T`` rows of a chunk; ``attend(qkv, att)`` launches the
        attention, None: the fused one (``_attn``); ``join``: ``_closing``'s"""
        rows, d = n * T, self.config.hidden_size
        qkv, att, y = self._rows(ws, "qkv", rows, 3 * d), self._rows(ws, "att", rows, d), self._rows(ws, "y", rows, d)
        ops.gemm(GEMM_NT, src, self._w(f"l{i}_qkv_w"), qkv, bias=self._f(f"l{i}_qkv_b"), epilogue=EPI_BIAS)
        if attend is None:
            self._attn(ws, qkv, att, n, T, T)
        else:
            attend(qkv, att)
        self._out_proj(i, att, resid, y, join)
        return y

    def _ffn(self, i: int, ws, src: torch.Tensor, resid: torch.Tensor, out: torch.Tensor, join: Optional[Join] = None,
             act: Optional[Act] = None) -> None:
        """out = resid + fc2(gelu(fc1(src) + b1)) + b2 on the rows of ``src``; ``join``: ``_closing``'s; ``act``: the model's own
        activation launch (in place here)"""
        h = self._rows(ws, "h", src.shape[0], self.config.intermediate_size)
        ops.gemm(GEMM_NT, src, self._w(f"l{i}_fc1_w"), h)
        if act is None:
            lib.bias_gelu(h, self._f(f"l{i}_fc1_b"))
        else:
            act[0](h, self._f(f"l{i}_fc1_b"), h)
        self._closing(i, "fc2", h, resid, out, join)

    def _post_ln_layer(self, i: int, ws, n: int, T: int, attend: Optional[Attend] = None, join: Optional[Join] = None,
                       act: Optional[Act] = None) -> None:
        """x = LayerNorm(ln + ffn(ln)), ln = LayerNorm(x + attention(x)) on the ``n * T`` rows of ``x``; ``join``: ``_closing``'s,
        ``act``: ``_ffn``'s"""
        rows, d = n * T, self.config.hidden_size
        x, ln = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d)
        y = self._attention(i, ws, x, x, n, T, attend, join)
        self._ln(ws, y, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        self._ffn(i, ws, ln, ln, y, join, act)
        self._ln(ws, y, x, f"l{i}_ln2_w", f"l{i}_ln2_b")

    def _post_ln_layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int, attend: Optional[Attend], attn_bwd: AttnBwd,
                            qkv_wgrad: Optional[QkvWgrad], below: bool = True, slabs: Optional[Callable[[int, int], int]] = None,
                            join: Optional[Join] = None, join_bwd: Optional[JoinBwd] = None, act: Optional[Act] = None) -> None:
        """``_post_ln_layer`` ``i`` again from its saved input ``xin``, then its backward (the module docstring has the rows):
        ``ga`` holds the gradient of the layer's output on entry and, with ``below``, of ``xin`` on return.  ``attend`` as in
        ``_attention``; it leaves the lse where ``attn_bwd(qkv, att, datt, dqkv)`` reads it.  With ``qkv_wgrad(dqkv, xin)`` the
        layer trains: its weight, bias and LayerNorm gradients are added into the parameters' ``.grad``, the four plain weights'
        in ``slabs(rows, tiles)`` K-slabs (``_slabs_for``; None: plain launches).  Without, no weight gradient is formed.
        ``join`` / ``join_bwd`` (both or neither): the forward's ``_closing`` hook and its gradient.  The gradient of a pre-LN sum
        then reaches the residual branch as it is and the dense branch (the closing launch's weight and input gradients) as
        ``join_bwd(role, dy, out)`` leaves it in ``out``: the second pre-LN sum's buffer, which is free once LayerNorm 2's backward
        has read it.  ``act`` = (forward, backward): the model's own activation launches in place of ``bias_gelu_to`` /
        ``bias_gelu_bwd``, with their arguments (Wav2Vec2's activation dropout); None: those two"""
        c = self.config
        gelu_to, gelu_bwd = (lib.bias_gelu_to, lib.bias_gelu_bwd) if act is None else act
        rows, d, I, R, train = n * T, c.hidden_size, c.intermediate_size, self._rows, qkv_wgrad is not None
        ga, gb, dh, dqkv, y2, gel = R(g, "ga", rows, d), R(g, "gb", rows, d), R(g, "dh", rows, I), R(g, "dqkv", rows, 3 * d), R(g, "y2", rows, d), R(g, "g", rows, I)
        ln, h, qkv, att = R(ws, "ln", rows, d), R(ws, "h", rows, I), R(ws, "qkv", rows, 3 * d), R(ws, "att", rows, d)
        st1, st2 = self._stats(g, 1), self._stats(g, 2)
        W, F = lambda r: self._w(f"l{i}_{r}_w"), lambda r: self._f(f"l{i}_{r}_b")

        def wgrad(dy: torch.Tensor, x: torch.Tensor, r: str, M: int, N: int) -> None:
            if train:
                self._wgrad(dy, x, f"l{i}_{r}", slabs(rows, self._tiles(M, N)) if slabs else 1)
        # the forward again: both LayerNorms' statistics, the raw fc1 output and the GELU output side by side
        def dense_grad(role: str, dy: torch.Tensor) -> torch.Tensor:
            if join_bwd is None:
                return dy
            join_bwd(role, dy, y2)
            return y2
        y1 = self._attention(i, ws, xin, xin, n, T, attend, join)
        self._ln(st1, y1, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        ops.gemm(GEMM_NT, ln, W("fc1"), h)
        gelu_to(h, F("fc1"), gel)
        self._closing(i, "fc2", gel, ln, y2, join)
        self._ln(st2, y2, R(ws, "x", rows, d), f"l{i}_ln2_w", f"l{i}_ln2_b")          # for its statistics; the output is not read
        # the MLP
        self._ln_bwd(st2, y2, ga, gb, f"l{i}_ln2_w", self._grads(i, "ln2") if train else None)          # gb = dy2
        gd = dense_grad("fc2", gb)
        wgrad(gd, gel, "fc2", d, I)
        ops.gemm(GEMM_NN, gd, W("fc2"), dh)                                           # dg
        gelu_bwd(dh, h, F("fc1"), dh)
        wgrad(dh, ln, "fc1", I, d)
        ops.gemm(GEMM_NN, dh, W("fc1"), ga, aux=gb, epilogue=EPI_ADD_AUX)             # ga = dln1: the MLP branch + the residual
        # the attention
        self._ln_bwd(st1, y1, ga, gb, f"l{i}_ln1_w", self._grads(i, "ln1") if train else None)          # gb = dy1
        gd = dense_grad("o", gb)
        wgrad(gd, att, "o", d, d)
        ops.gemm(GEMM_NN, gd, W("o"), ga)                                             # ga = datt
        attn_bwd(qkv, att, ga, dqkv)
        if train:
            qkv_wgrad(dqkv, xin)
        if below:
            ops.gemm(GEMM_NN, dqkv, W("qkv"), ga, aux=gb, epilogue=EPI_ADD_AUX)       # ga = dx: the attention branch + the residual

    def _pre_ln_layer(self, i: int, ws, n: int, T: int) -> None:
        """x = y + ffn(LayerNorm(y)), y = x + attention(LayerNorm(x)) on the ``n * T`` rows of ``x`` (ViT; Wav2Vec2's layer-norm
        family; Whisper's encoder)"""
        rows, d = n * T, self.config.hidden_size
        x, ln = self._rows(ws, "x", rows, d), self._rows(ws, "ln", rows, d)
        self._ln(ws, x, ln, f"l{i}_ln1_w", f"l{i}_ln1_b")
        y = self._attention(i, ws, ln, x, n, T)
        self._ln(ws, y, ln, f"l{i}_ln2_w", f"l{i}_ln2_b")
        self._ffn(i, ws, ln, y, x)

    def _pre_ln_layer_grad(self, i: int, ws, g, xin: torch.Tensor, n: int, T: int, attn_bwd: AttnBwd, qkv_wgrad: QkvWgrad,
                           slabs: Callable[[int, int], int]) -> None:
        """``_pre_ln_layer`` ``i`` again from its saved input ``xin`` up to the GELU output (nothing behind fc2 is read by a pre-LN
        layer's backward), then its backward with the weight, bias and LayerNorm gradients added into the parameters' ``.grad``, on
        a ``_grad_rows(T, "ln2")`` workspace: ``ga`` holds the gradient of the layer's output on entry and of ``xin`` on return.
        ``attn_bwd(qkv, att, datt, dqkv)`` and ``qkv_wgrad(dqkv, ln1)`` are the model's; the four plain weights' gradients take
        ``slabs(rows, tiles)`` K-slabs.  The Q/K/V input gradient is always formed: the first LayerNorm's own parameter gradients
        come out of its backward, whether or not anything below the layer trains"""
        c = self.config
        d, I, R, rows = c.hidden_size, c.intermediate_size, self._rows, n * T
        ln1, qkv, dqkv = R(ws, "ln", rows, d), R(ws, "qkv", rows, 3 * d), R(g, "dqkv", rows, 3 * d)
        att, h, ln2, gel, ga, gb, dh = R(ws, "att", rows, d), R(ws, "h", rows, I), R(g, "ln2", rows, d), R(g, "g", rows, I), R(g, "ga", rows, d), R(g, "gb", rows, d), R(g, "dh", rows, I)
        st1, st2 = self._stats(g, 1), self._stats(g, 2)
        S = lambda M, N: slabs(rows, self._tiles(M, N))
        W, F = lambda r: self._w(f"l{i}_{r}_w"), lambda r: self._f(f"l{i}_{r}_b")
        self._ln(st1, xin, ln1, f"l{i}_ln1_w", f"l{i}_ln1_b")
        y = self._attention(i, ws, ln1, xin, n, T)
        self._ln(st2, y, ln2, f"l{i}_ln2_w", f"l{i}_ln2_b")
        ops.gemm(GEMM_NT, ln2, W("fc1"), h)
        lib.bias_gelu_to(h, F("fc1"), gel)
        # the MLP
        self._wgrad(ga, gel, f"l{i}_fc2", S(d, I))
        ops.gemm(GEMM_NN, ga, W("fc2"), dh)                                            # dg
        lib.bias_gelu_bwd(dh, h, F("fc1"), dh)
        self._wgrad(dh, ln2, f"l{i}_fc1", S(I, d))
        ops.gemm(GEMM_NN, dh, W("fc1"), gb)                                            # dln2
        self._ln_bwd(st2, y, gb, ga, f"l{i}_ln2_w", self._grads(i, "ln2"), resid=ga)   # ga = dy: the MLP branch + the residual
        # the attention
        self._wgrad(ga, att, f"l{i}_o", S(d, d))
        ops.gemm(GEMM_NN, ga, W("o"), gb)                                              # datt
        attn_bwd(qkv, att, gb, dqkv)
        qkv_wgrad(dqkv, ln1)
        ops.gemm(GEMM_NN, dqkv, W("qkv"), gb)                                          # dln1
        self._ln_bwd(st1, xin, gb, ga, f"l{i}_ln1_w", self._grads(i, "ln1"), resid=ga)  # ga = dx: the attention branch + the residual

    @staticmethod
    def _widen(src: torch.Tensor, dst: torch.Tensor) -> None:
        lib.check(lib.load().mmf_cast_bf16_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), lib.stream_ptr()))

    @staticmethod
    def _narrow(src: torch.Tensor, dst: torch.Tensor) -> None:
        """contiguous f32 -> bf16, one rounding (an incoming gradient)"""
        lib.check(lib.load().mmf_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(), lib.stream_ptr()))
