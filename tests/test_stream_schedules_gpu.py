"""The multi-stream schedules of the default eager configuration against their serial replay (tests/stream_sched.py).

Per case, from identical restored state (parameters, bf16 shadow, gradient arena, optimiser state, dropout state, and the host
side of the deferred wgrad queue):

  S     the step under ``serial_replay()``: the same launches in the same host order, all on one stream — the reference;
  C     the step on the default streams, under the launch census, event-timed;
  D_k   the step on the default streams with ONE on-device sleep in front of launch k, for EVERY boundary k of the census (a
        launch whose stream differs from its predecessor's or successor's, the first launch of backward, the first launch of
        the wgrad flush).  The sleep is 5 x the measured time of C, at most 50 ms.

S is compared with C and with every D_k.  Snapshots are cloned on the main stream right behind the step with NO device-wide
synchronisation in front, as the next step of a training loop would read them.  A dropped join is wrong only when the producer
stream is late, and a missing ``record_stream`` only when the block is handed out again early: the sleep makes the first
deterministic, the ``no_grad`` case with preloaded allocator pools exposes the second.

What must be bit-equal: every tensor whose elements have one writer each — every output, every input gradient, every weight
gradient.  The launches, their arguments and their order of issue are the same in S, C and D_k.  What may differ between two
runs of the SAME schedule is what float atomics accumulate (EXEMPT below, each with the line of its atomic); those are held to
the bounds tests/helpers.py ``check_graph_replay_matches_eager`` holds "same launches, other schedule" to: loss 1e-6 relative,
gradients 1e-6 of the arena's maximum, parameters 1e-6 absolute.  In a training run the masters are downstream of the clipped
update (``gnorm_sq``) and take the parameter bound; every step starts from the serial replay's state (case 4).

All runs are eager; no graph is captured here (graphs with parallel branches crash on these machines, bench.single_stream), no
stream is created beyond the product's own, no queue-related environment is set.

Measured on an MI355X: profiles/stream_schedule_parity.txt."""
import re
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_sched as ss  # noqa: E402
from helpers import l2_rel, relu_agreement  # noqa: E402
from mmfusion import synth  # noqa: E402

LOSS_REL, GRAD_OF_MAX, PARAM_ABS = 1e-6, 1e-6, 1e-6     # check_graph_replay_matches_eager's bounds
MAX_BOUNDARIES = 64

# Parameter gradients accumulated by float atomics: (name pattern, class of the module that owns the parameter, the atomic), one
# entry per producer.  Everything else in the arena is bit-equal — a bias that a single-writer kernel produces included.
EXEMPT_GRADS = [
    (r"(.*\.)?bias", "Linear", "nn.Linear bias = column sums of dy: csrc/gemm6.hip:280 and gemm2.hip:252 (wgrad epilogue), "
                               "elementwise.hip:277 (colsum) - whichever of the three the launch takes; every nn.Linear of these models gets its bias "
                               "gradient from one of them, and one that got it from a single-writer kernel would ride in under this entry"),
    (r"(.*\.)?in_proj_bias", "_MHAParams", "attention in-projection bias, the same column sums: csrc/gemm6.hip:280, gemm2.hip:252, "
                                           "elementwise.hip:277"),
    (r"(.*\.)?norm[12]\.bias", "LayerNorm", "LayerNorm dbeta: csrc/layernorm.hip:434"),
    (r"(.*\.)?norm[12]\.weight", "LayerNorm", "LayerNorm dgamma: csrc/layernorm.hip:433"),
    (r".*gcn_layers\.\d+\.bias", "_DenseGAT", "GAT bias: csrc/small.hip:189"),
    (r".*gcn_layers\.\d+\.att_(src|dst)", "_DenseGAT", "GAT attention vectors: csrc/small.hip:204-205"),
    (r".*weight_predictor\.2\.bias", "Linear", "adaptive-combine d -> 3 bias: csrc/small.hip:438 (also under the first entry)"),
    (r".*weight_predictor\.2\.weight", "Linear", "adaptive-combine d -> 3 weight: csrc/small.hip:447"),
]
# Outputs accumulated by float atomics.
EXEMPT_OUTPUTS = [
    (r"contrastive_losses\..*", "InfoNCE value: 2 B terms added into one LDS float, csrc/small.hip:300 (its gradient does not read it)"),
]


def _say(line):
    print("stream-sched: " + line)


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    """the file's wall time, for profiles/stream_schedule_parity.txt"""
    t0 = time.time()
    yield
    _say(f"wall time of tests/test_stream_schedules_gpu.py: {time.time() - t0:.1f} s")


def _matches(name, table):
    return any(re.fullmatch(p, name) for p, _ in table)


def _exempt_grad(name, owner):
    return any(re.fullmatch(p, name) and type(owner).__name__ == cls for p, cls, _ in EXEMPT_GRADS)


def _exempt_mask(arena, module):
    mask = torch.zeros(arena.numel, dtype=torch.bool, device=arena.grads.device)
    where = {id(p): i for i, p in enumerate(arena.params)}
    names = []
    for mn, sub in module.named_modules():
        for pn, p in sub.named_parameters(recurse=False):
            n = f"{mn}.{pn}" if mn else pn
            if _exempt_grad(n, sub):
                o = arena.offsets[where[id(p)]]
                mask[o:o + p.numel()] = True
                names.append(n)
    return mask, names


def _roles():
    from mmfusion import ops
    out = {torch.cuda.current_stream().cuda_stream: "main"}
    for i, s in enumerate(ops._branch_streams):
        out[s.cuda_stream] = f"branch{i}"
    if ops._wgrad_stream is not None:
        out[ops._wgrad_stream.cuda_stream] = "wgrad"
    return out


class Case:
    """One schedule under test.  Subclasses set: name, arena, module, uses (stream roles the census must show), training,
    state (device tensors restored before every run) and implement step(mark) -> {key: tensor} (clones, no device sync)."""
    delay_steps = None                       # training runs of several steps: delays only in these (1-based) steps
    serial = False                           # set by check_case around the run under serial_replay()

    def restore(self, saved):
        from mmfusion import ops
        torch.cuda.synchronize()
        for x, v in zip(self.state, saved):
            x.copy_(v)
        ops._bw = ops._Backward()            # the host side of the deferred wgrad queue: nothing learned from an earlier backward
        ops._pending_wgrad.clear()
        torch.cuda.synchronize()

    def kind(self, key):
        """'equal' | 'grads' (bit-equal outside the exempt mask, 1e-6 of max inside) | 'loss' | 'param'"""
        raise NotImplementedError


def _compare(case, ref, got, tag, stats, failures):
    for key, want in ref.items():
        have, kind = got[key], case.kind(key)
        if kind == "equal":
            ok = torch.equal(want, have)
            if ok:
                stats["equal"] += 1
            else:
                failures.append(f"{tag}: {key} not bit-equal, max |diff| {float((want.float() - have.float()).abs().max()):.3e}")
            continue
        d = (want.double() - have.double()).abs()
        if kind == "grads":
            strict_bad = (want != have) & ~case.mask
            if bool(strict_bad.any()):
                bad = [n for n, g in case.grad_views() if bool(strict_bad[g[0]:g[1]].any())]
                failures.append(f"{tag}: {key}: single-writer gradients not bit-equal: {bad[:8]}{' ...' if len(bad) > 8 else ''}, "
                                f"max |diff| {float(d[strict_bad].max()):.3e}")
            else:
                stats["equal"] += 1
            err, bound = float(d[case.mask].max()) if bool(case.mask.any()) else 0.0, GRAD_OF_MAX * float(want.abs().max())
        elif kind == "loss":
            err, bound = float(d.max()), LOSS_REL * max(1.0, float(want.abs().max()))
        elif kind == "param":
            err, bound = float(d.max()), PARAM_ABS
        else:
            raise KeyError(kind)
        if not err <= bound:                                      # (NaN fails)
            failures.append(f"{tag}: {key} ({kind}) differs by {err:.3e}, bound {bound:.3e}")
        w = stats["worst"].setdefault(f"{key} ({kind})", [0.0, bound])
        if err / max(bound, 1e-300) >= w[0] / max(w[1], 1e-300):
            w[0], w[1] = err, bound


def check_case(case):
    """S against C and against every D_k; returns the census and the statistics."""
    from mmfusion import ops
    t0 = time.time()
    sleeper = ss.sleeper()
    noop = lambda label: None
    case.step(noop)                                               # warm-up: streams exist, the allocator pools are filled,
    case.step(noop)                                               # the arena knows its wgrad-managed regions
    torch.cuda.synchronize()
    saved = [x.clone() for x in case.saved_from()]
    main = torch.cuda.current_stream()

    with ss.serial_replay():
        case.restore(saved)
        case.serial = True
        try:
            S = case.step(noop)
        finally:
            case.serial = False
        torch.cuda.synchronize()
    assert not any(bool(v.isnan().any()) for v in S.values()), "NaN in the serial replay"

    case.restore(saved)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with ss.launch_census() as census:
        e0.record(main)
        C = case.step(census.mark)
        ops.join_branch_streams()
        if ops._wgrad_stream is not None:
            main.wait_stream(ops._wgrad_stream)
        e1.record(main)
        torch.cuda.synchronize()
    t_c = float(e0.elapsed_time(e1))
    sleep_ms = min(5.0 * t_c, ss.SLEEP_CAP_MS)

    stats, failures = {"equal": 0, "worst": {}}, []
    _compare(case, S, C, "C", stats, failures)

    roles = _roles()
    by_role = {}
    for s in census.streams:
        by_role[roles.get(s, hex(s))] = by_role.get(roles.get(s, hex(s)), 0) + 1
    starts = census.starts("bwd.*", "flush")
    bounds = ss.boundaries(census.streams, starts)
    if case.delay_steps is not None:
        bounds = [k for k in bounds if case.step_of(census, k) in case.delay_steps]
    assert len(bounds) <= MAX_BOUNDARIES, f"{len(bounds)} boundaries: shrink the case, not the list"

    def phase(k):
        p = census.phase(k) or ""
        return "forward" if p.startswith("fwd") else "backward"
    # non-vacuity: the streams this case is about carry launches, and are held back in the forward and in the backward
    delayed = {(roles.get(census.streams[k]), phase(k)) for k in bounds}
    for role in case.uses:
        assert by_role.get(role, 0) > 0, f"no launch on {role}: {by_role}"
        in_steps = [k for k in range(len(census.streams)) if roles.get(census.streams[k]) == role
                    and (case.delay_steps is None or case.step_of(census, k) in case.delay_steps)]
        assert in_steps, f"no launch on {role} in steps {case.delay_steps}"
        phases = ("backward",) if role == "wgrad" else ("forward", "backward") if case.training else ("forward",)
        for ph in phases:
            assert (role, ph) in delayed, f"no delay on {role} in the {ph}: {sorted(delayed)}"

    for k in bounds:
        case.restore(saved)
        with ss.delayed_launch(k, lambda s: sleeper.enqueue(sleep_ms)) as fired:
            e0.record(main)
            D = case.step(noop)
            ops.join_branch_streams()
            if ops._wgrad_stream is not None:
                main.wait_stream(ops._wgrad_stream)
            e1.record(main)
            torch.cuda.synchronize()
        assert fired == [census.streams[k]], f"launch {k} went to another stream than in the census"
        # the delay did delay: this run, event-timed as C was, took at least half its sleep
        t_d = float(e0.elapsed_time(e1))
        assert t_d >= 0.5 * sleep_ms, f"D_{k} ran {t_d:.2f} ms on the device with a sleep of {sleep_ms:.1f} ms in it"
        _compare(case, S, D, f"D_{k} [{roles.get(census.streams[k])}, {census.phase(k)}]", stats, failures)

    _say(f"{case.name}: launches {len(census.streams)} {by_role}, boundaries {len(bounds)}, C {t_c:.2f} ms, sleep {sleep_ms:.1f} ms "
         f"({sleeper.kind}, {sleeper.check:.1f} ms measured for 5), bit-equal tensor comparisons {stats['equal']}, runs 1 S + 1 C + {len(bounds)} D, {time.time() - t0:.1f} s")
    for key, (err, bound) in sorted(stats["worst"].items()):
        _say(f"{case.name}:     {key}: worst {err:.3e} / bound {bound:.3e}")
    assert not failures, f"{case.name}: {len(failures)} mismatches against the serial replay:\n  " + "\n  ".join(failures[:40])
    return census, stats, S


# ---- cases 1 and 2: MultimodalTransformer as the root module ---------------------------------------------------------------
def _cfg(d, H, p, G=None, L=3):
    import config as cfgmod
    cfg = cfgmod.ModelConfig()
    cfg.fusion_hidden_size, cfg.fusion_num_heads = d, H
    cfg.graph_hidden_size, cfg.graph_num_layers = G or d, L
    cfg.fusion_dropout = cfg.graph_dropout = p
    return cfg


class _Probe:
    """synth.probe_loss with its cotangents resident on the device (probe_loss builds them on the host and copies them in
    every call, which makes the host wait for the forward; a training loop does not)."""

    def __init__(self):
        self.p = {}

    def __call__(self, out):
        total = None
        for k, v in synth.flatten_outputs(out).items():
            if k.rsplit(".", 1)[-1] in synth.NON_DIFF_KEYS or not v.is_floating_point():
                continue
            if k not in self.p:
                self.p[k] = synth.probe_vector("out:" + k, v.numel()).reshape(v.shape).to(device=v.device)
            term = (v.float() * self.p[k]).sum()
            total = term if total is None else total + term
        return total


class ModuleCase(Case):
    """forward (+ probe-loss backward) of one fusion module"""

    def __init__(self, name, module, xs, uses, training, kwargs=None, out_mask=None, forwards=1):
        from mmfusion import arena as arena_mod, ops
        self.name, self.module, self.uses, self.training = name, module, uses, training
        self.x0, self.kwargs, self.out_mask, self.forwards = [x.cuda() for x in xs], kwargs or {}, out_mask, forwards
        self.arena = arena_mod.ensure(module)
        self.probe = _Probe()
        self.mask, self.exempt_names = _exempt_mask(self.arena, module)
        a = self.arena
        self.state = [a.master_full, a.shadow_full, a.grads_full, ops.rng_state()]

    def saved_from(self):
        self.arena.grads_full.zero_()
        return self.state

    def grad_views(self):
        where = {id(p): i for i, p in enumerate(self.arena.params)}
        for n, p in self.module.named_parameters():
            o = self.arena.offsets[where[id(p)]]
            yield n, (o, o + p.numel())

    def masked(self, out):
        if self.out_mask is None:
            return out
        out = dict(out)
        out["fused_features"] = out["fused_features"] * self.out_mask
        return out

    def step(self, mark):
        snap = {}
        if not self.training:
            with torch.no_grad():
                for i in range(self.forwards):
                    mark(f"fwd{i + 1}")
                    out = self.module(*self.x0, **self.kwargs)
                    for k, v in synth.flatten_outputs(out).items():
                        snap[f"out{i + 1}.{k}"] = v.clone()
            return snap
        xs = [x.detach().clone().requires_grad_(True) for x in self.x0]
        mark("fwd1")
        out = self.module(*xs, **self.kwargs)
        loss = self.probe(self.masked(out))
        mark("bwd1")
        loss.backward()
        for k, v in synth.flatten_outputs(out).items():
            snap["out." + k] = v.detach().clone()
        for i, x in enumerate(xs):
            snap[f"gin.{i}"] = x.grad.clone()
        snap["grads"] = self.arena.grads.clone()
        return snap

    def step_of(self, census, k):
        return 1

    def kind(self, key):
        if key == "grads":
            return "grads"
        if _matches(key.split(".", 1)[1], EXEMPT_OUTPUTS):
            return "loss"
        return "equal"


TS = (24, 20, 6)


def _mult(d, p, train):
    from models import fusion_layers as fl
    torch.manual_seed(synth.WEIGHT_SEED)
    m = fl.MultimodalTransformer(_cfg(d, 2, p))
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    return (m.train() if train else m.eval()), state


@pytest.mark.parametrize("d,p", [(128, 0.0), (128, 0.1), (192, 0.0), (192, 0.1)])
def test_root_mult_training_step_matches_its_serial_replay(d, p):
    """Case 1: root MulT, B = 2, T = 24 / 20 / 6, H = 2 (head_dim 64 and 96): the text chain on the current stream, audio +
    video on branch stream 1, forward and backward.  At d = 128, p = 0 the serial replay itself is held to the bf16-storage
    oracle at test_parity_gpu.py's OUT_BF16 / GIN_L2_BF16 / GP_L2_BF16, flip-aware as the bench-configuration test is: the
    fused_features units whose ReLU state differs between the two sides are left out of the probe loss on both."""
    from test_parity_gpu import GIN_L2_BF16, GP_L2_BF16, OUT_BF16
    from oracle import ref_cpu
    m, state = _mult(d, p, True)
    xs = synth.make_features(2, TS, d)
    oracle = d == 128 and p == 0.0
    mask = None
    if oracle:
        with ref_cpu.bf16_storage(), torch.no_grad():
            ref0 = ref_cpu.multimodal_transformer(state, "", *xs, 2)
        with torch.no_grad():
            out0 = m(*[x.cuda() for x in xs])
        agree, nflip, bound = relu_agreement(out0["fused_features"], ref0["fused_features"], "fused_features")
        mask = agree
    case = ModuleCase(f"case 1 MulT root d={d} p={p}", m, xs, ["branch1"], True, out_mask=None if mask is None else mask.cuda())
    census, stats, S = check_case(case)
    if oracle:
        Pb = {k: v.clone().requires_grad_(True) for k, v in state.items()}
        xb = [x.clone().requires_grad_(True) for x in xs]
        with ref_cpu.bf16_storage():
            ref = ref_cpu.multimodal_transformer(Pb, "", *xb, 2)
            ref_m = dict(ref)
            ref_m["fused_features"] = ref["fused_features"] * mask
            synth.probe_loss(ref_m).backward()
        worst = [0.0, 0.0, 0.0]
        for k, want in ref.items():
            worst[0] = max(worst[0], l2_rel(S["out." + k], want))
            assert l2_rel(S["out." + k], want) <= OUT_BF16, f"serial replay: {k} vs bf16-storage oracle {l2_rel(S['out.' + k], want):.3e}"
        for i, r in enumerate(xb):
            worst[1] = max(worst[1], l2_rel(S[f"gin.{i}"], r.grad))
            assert l2_rel(S[f"gin.{i}"], r.grad) <= GIN_L2_BF16, f"serial replay: input grad {i} {l2_rel(S[f'gin.{i}'], r.grad):.3e}"
        for n, (o, e) in case.grad_views():
            want = Pb[n].grad
            if want is None or float(want.abs().max()) == 0.0:
                continue
            err = l2_rel(S["grads"][o:e].view(want.shape), want)
            worst[2] = max(worst[2], err)
            assert err <= GP_L2_BF16, f"serial replay: param grad {n} vs bf16-storage oracle {err:.3e}"
        _say(f"{case.name}:     serial replay vs bf16-storage oracle: outputs {worst[0]:.2e} (<= {OUT_BF16}), input grads "
             f"{worst[1]:.2e} (<= {GIN_L2_BF16}), param grads {worst[2]:.2e} (<= {GP_L2_BF16}); {nflip} ReLU flips masked")


@pytest.mark.parametrize("d", [128, 192])
def test_root_mult_no_grad_forward_matches_its_serial_replay(d):
    """Case 2: the same module in eval mode under no_grad, two forwards back to back per run.  Nothing keeps an activation
    alive here, so a block goes back to the caching allocator the moment its tensor dies; the pools are preloaded (the
    warm-up forwards, plus blocks of the activations' sizes allocated and freed on the main stream), so a freed block is
    handed out again at once.  This is the case that sees a block reused while another stream still reads it."""
    m, _ = _mult(d, 0.0, False)
    xs = synth.make_features(2, TS, d)
    case = ModuleCase(f"case 2 MulT root no_grad d={d}", m, xs, ["branch1"], False, forwards=2)
    for T in TS:
        for width in (1, 3, 4):
            blocks = [torch.empty(2 * T * d * width, dtype=torch.bfloat16, device="cuda") for _ in range(4)]
            del blocks
    check_case(case)


# ---- case 3: HierarchicalFusion ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inputs", ["seq", "rows"])
def test_hierarchical_fusion_matches_its_serial_replay(inputs):
    """Case 3: B = 3, d = 128, H = 2, training mode with dropout 0.1, contrastive losses on.  'seq': (B, T, d) inputs, the four
    small branches issued on branch stream 0 between the stages of the nested MulT (the `_between` thunks).  'rows': (B, d)
    inputs, the `rows_only` order (all four branches up front)."""
    from models import fusion_layers as fl
    torch.manual_seed(synth.WEIGHT_SEED)
    m = fl.HierarchicalFusion(_cfg(128, 2, 0.1)).cuda().train()
    xs = synth.make_features(3, TS if inputs == "seq" else (0, 0, 0), 128)
    case = ModuleCase(f"case 3 Hier {inputs}", m, xs, ["branch0"], True, kwargs={"compute_contrastive_loss": True})
    check_case(case)


# ---- case 4: the training step -----------------------------------------------------------------------------------------------------
class TrainCase(Case):
    """three consecutive FusionTrainStep steps: lazy zeroing, finalize_grads, FusedAdamW with clipping"""
    training = True

    def __init__(self, name, ts, module, xs, labels, uses, delay_step):
        from mmfusion import ops
        self.name, self.ts, self.module, self.uses = name, ts, module, uses
        self.arena, self.xs, self.labels, self.delay_steps = ts.arena, xs, labels, (delay_step,)
        a, opt = ts.arena, ts.opt
        self.mask, self.exempt_names = _exempt_mask(a, module)
        self.state = [a.master_full, a.shadow_full, a.grads_full, opt.exp_avg, opt.exp_avg_sq, opt.step_dev, opt.hparams, opt.gnorm_sq,
                      ops.rng_state()]
        # what one step hands to the next through the optimiser: masters, shadow, moments, step count, gnorm_sq.  The gradient
        # arena is NOT among them (lazy zeroing: step i + 1 overwrites it and never reads step i's), so a late write into it from
        # a stream that step i failed to join stays visible in step i + 1.
        self.carried = [a.master_full, a.shadow_full, opt.exp_avg, opt.exp_avg_sq, opt.step_dev, opt.gnorm_sq]
        self.carry = {}

    def saved_from(self):
        return self.state

    grad_views = ModuleCase.grad_views

    def step(self, mark):
        from mmfusion import train as train_mod
        snap = {}

        def marking(orig):
            def backward_from(loss):
                mark(f"bwd{self.i}")
                return orig(loss)
            return backward_from
        with ss._wrapped(train_mod, "backward_from", marking):
            for self.i in (1, 2, 3):
                mark(f"fwd{self.i}")
                loss = self.ts(*self.xs, self.labels)
                snap[f"step{self.i}.loss"] = loss.detach().clone()
                snap[f"step{self.i}.grads"] = self.arena.grads.clone()
                snap[f"step{self.i}.master"] = self.arena.master.clone()
                if self.i < 3:
                    if self.serial:
                        self.carry[self.i] = [x.clone() for x in self.carried]
                    for x, v in zip(self.carried, self.carry.get(self.i, ())):      # (in S too: one host path; none in the warm-up)
                        x.copy_(v)           # on the main stream, behind the snapshots, with no synchronisation
        return snap

    def step_of(self, census, k):
        return sum(1 for label, k0 in census.marks if label.startswith("fwd") and k0 <= k)

    def kind(self, key):
        step, what = key.split(".")
        if what == "loss":
            return "loss"                    # (the contrastive terms: EXEMPT_OUTPUTS)
        if what == "master":
            return "param"                   # every update is scaled by the clip factor, a function of gnorm_sq (csrc/optim.hip:61)
        return "grads"                       # every step starts from the serial replay's state: bit-equal outside the exempt list


def _train_case(early, delay_step, eps=1e-4):
    from mmfusion import arena as arena_mod, ops
    from mmfusion.train import FusedAdamW, FusionTrainStep
    from models import fusion_layers as fl
    from models.multimodal_model import EmotionClassifier
    cfg = _cfg(128, 2, 0.1)
    torch.manual_seed(synth.WEIGHT_SEED)
    fusion, head = fl.HierarchicalFusion(cfg), EmotionClassifier(cfg)

    class FusionWithHead(fl._FusionBase):
        def __init__(self):
            super().__init__()
            self.fusion_layer, self.classifier = fusion, head

        def forward(self, t, a, v, compute_contrastive_loss=False):
            return self.fusion_layer(t, a, v, compute_contrastive_loss=compute_contrastive_loss)
    model = FusionWithHead().cuda().train()
    ar = arena_mod.ensure(model)
    # Adam's eps is 1e-4 here, not the default 1e-8.  Some gradients cancel exactly in exact arithmetic (the key bias of a softmax
    # attention) and are, as computed, nothing but the rounding noise of their atomics' order, 1e-10 ... 1e-8; Adam divides by
    # sqrt(v) + eps, so with eps below the noise their update is +-lr whichever way the noise fell, WITHIN one step and between
    # two runs of one schedule (profiles/stream_schedule_parity.txt, "drift", eps=1e-08: masters lr apart).  With eps = 1e-4 a
    # gradient difference delta moves an update by at most lr * delta / eps = 1e-3 * 1e-8 / 1e-4 = 1e-7, inside the 1e-6 bound,
    # while a gradient that is wrong by its own size still moves its parameter by ~lr = 1e-3 (typical |g| after clipping
    # 1 / sqrt(numel) = 6e-4 > eps).
    opt = FusedAdamW(ar, lr=1e-3, eps=eps, weight_decay=1e-5, max_grad_norm=1.0)
    opt.set_schedule(1e-3, 20)               # OneCycle over 20 steps: 4e-5 in step 1, 1e-3 from step 2 on
    ts = FusionTrainStep(model, model.classifier, ar, lr=1e-3, total_steps=20, opt=opt)
    xs = [x.cuda() for x in synth.make_features(3, TS, 128)]
    labels = torch.randint(0, 7, (3,), generator=torch.Generator().manual_seed(99)).cuda()
    return TrainCase(f"case 4 train early={early} delays in step {delay_step}", ts, model, xs, labels,
                     ["branch0", "wgrad"] if early else ["branch0"], delay_step)


@pytest.mark.parametrize("delay_step", [2, 3])
@pytest.mark.parametrize("early", [False, True])
def test_training_steps_match_their_serial_replay(early, delay_step):
    """Case 4: FusionTrainStep over HierarchicalFusion + classifier head at the case-3 size, three consecutive steps per run
    (lazy zeroing, finalize_grads, FusedAdamW, clipping on), loss / gradient arena / masters after every step.  The delays go
    into step 2 and step 3 (one parametrised test each: a step has some 40 boundaries).  early: ops._WGRAD_EARLY on — the
    early wgrad launch fires from the second backward of a run on (the first has no count to go by), on the wgrad stream; the
    census must show it there.

    Every step of C and of every D_k starts from the serial replay's state: behind a step's snapshots, what the optimiser hands
    to the next step (masters, shadow, moments, step count, gnorm_sq) is overwritten with S's, on the main stream and with no
    synchronisation; S copies its own values the same way, so the host path is one.  Each step is therefore compared on its own:
    its gradients are bit-equal outside the exempt list, as in step 1.  Without this the comparison is not deterministic: a
    master one ulp apart after a step (the clip factor's gnorm_sq atomics) now and then falls on the other side of a bf16
    rounding of the shadow, and the next step's gradients are then up to 9e-5 of their maximum apart — between two runs of
    ONE schedule, serial against serial as well (profiles/stream_schedule_parity.txt, "drift").  The gradient arena is not
    overwritten (lazy zeroing: the next step never reads it), so a late write into it by an unjoined stream still shows."""
    from mmfusion import ops
    case = _train_case(early, delay_step)
    saved_early = ops._WGRAD_EARLY
    ops._WGRAD_EARLY = early
    try:
        census, stats, S = check_case(case)
    finally:
        ops._WGRAD_EARLY = saved_early
    roles = _roles()
    on_wgrad = [case.step_of(census, k) for k, s in enumerate(census.streams) if roles.get(s) == "wgrad"]
    assert (sorted(set(on_wgrad)) == [2, 3]) if early else not on_wgrad, f"launches on the wgrad stream in steps {sorted(set(on_wgrad))}"
    assert len({float(S[f"step{i}.loss"]) for i in (1, 2, 3)}) == 3          # new dropout masks every step
    assert float((S["step3.master"] - S["step1.master"]).abs().max()) > 0     # the parameters moved
