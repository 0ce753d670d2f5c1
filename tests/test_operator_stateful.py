"""Property test of the operator's HOST state machine: random sequences of what a serving process does to a Llama MLP
block - forwards at changing batch sizes, inputs that grow new outlier columns, load_state_dict, .half(), deepcopy, state_dict reads,
the joint gate / up route switched on and off, a layer called on its own - against a TWIN of the same block that keeps nothing between
forwards (every caching feature of MixqConfig off: no kept argument blocks, no joint image, no compaction, no kept outlier maps, no row
maxima handed over).  Invariant after every step: both blocks return the same bytes and hold the same reference-visible state
(`ind`, `weight_cache`, `cnt`, `add_outliers`, `forward_without_precondition_len`, state_dict) - a derived buffer that outlived what it
was made from would show as a different y.  The twin itself is held to the reference by the G5 / G8 fixtures.

Runs the PRODUCT modules (mixq_amd.linear / fused) on tests/backend_oracle.py: the oracle's arithmetic behind the real packed layouts, so
the code under test is the code that runs on the GPU; tests/test_gpu_round6.py has a short GPU twin of one fixed sequence.
Guards /root/reference/mixquant/modules/linear.py:165-289, :292-376 and fused/mlp.py:57-70 semantics under the caching this repo added.

ABI 1.6: the same machine in bfloat16 (BlockMachineBf16 / BlockMachine4Bf16: MixqConfig(act_dtype=bfloat16, fused_bf16, joint_gate_up_bf16,
w8a16_bf16) - the derived bf16 image of `weight_cache`, the bf16 `wo` of the joint image, the dtype suffix of the weight-only pack key), a
fourth member (an o_proj-like weight_only layer fed the block's output) and, on all four machines, `residual=` on every route (none,
contiguous, 3-D, row-strided; the kept plan's identity does not include the addend), the route switches fuse_down_amax / norm_kept_map /
joint_gate_up_bf16 flipped mid-life, and a per-layer load of gate_proj's outlier columns (4-bit layers: `ind` / `weight_cache` are
registered buffers only there).  The twin keeps nothing: besides its PLAIN config, everything its layers derive is dropped in front of
every call (MixLinear_GEMM's own `_Derived.invalidate`), so a derived buffer the product fails to rebuild is stale in the block alone.
That the net can fail is shown three ways: fixed_sequence_ext asserts the states it reaches, every machine counts the firings of each new
rule on a frozen block (derandomized: a fixed property), and four wrong products (monkeypatches) each make a machine raise."""
import collections
import copy

import numpy as np
import pytest
import torch
from conftest import swap_backend
from hypothesis import HealthCheck, Phase, settings, strategies as st
from hypothesis.stateful import RuleBasedStateMachine, initialize, invariant, precondition, rule, run_state_machine_as_test

import backend_oracle
import mixq_amd.fused as F
import mixq_amd.linear as L
from mixq_amd import FasterTransformerRMSNorm, MixLibCache, MixLinear_GEMM, MixLlamaMLP, MixqConfig

PLAIN = dict(compact_weights=False, one_call_forward=False, fuse_down_amax=False, joint_gate_up=False, norm_kept_map=False)
BF16 = torch.bfloat16
BF16_FLAGS = dict(act_dtype=BF16, fused_bf16=True, joint_gate_up_bf16=True, w8a16_bf16=True)     # (a bfloat16 block and its twin alike)


def _bits(t):
    return t.detach().contiguous().view(torch.int16) if t.dtype in (torch.float16, BF16) else t.detach()


def make_block(bit, K, I, seed, config, fp=32, dev="cpu", dtype=torch.float16):
    """[norm, MixLlamaMLP, o_proj]: the fused norm in front of up_proj, the MLP block, and a weight_only (W8A16) K -> K layer fed the block's
    output.  dtype=bfloat16: the layers are built from Linear(...).to(bfloat16) under a config with act_dtype=bfloat16."""
    g = torch.Generator().manual_seed(seed)
    mkw = lambda o, i: (torch.randn(o, i, generator=g) / (i ** 0.5)).half()
    lins = []
    for o, i in ((I, K), (I, K), (K, I)):
        l = torch.nn.Linear(i, o, bias=False).half()
        l.weight.data.copy_(mkw(o, i))
        lins.append(l.to(dtype))
    up, gate, down = lins
    cache = MixLibCache(32, bit=bit, device=dev, config=config)
    ls = torch.rand(K, generator=torch.Generator().manual_seed(seed + 1)) + 0.1 if bit == 4 else None
    mk = lambda l, b, s: MixLinear_GEMM.from_linear(l, b, cache=cache, layer_scales=s, dev=dev, fp_features_num=fp)
    up_q, gate_q, down_q = mk(up, bit, ls), mk(gate, bit, ls), mk(down, 8, None)
    norm = FasterTransformerRMSNorm((1 + 0.1 * torch.randn(K, generator=g)).half().to(dev), eps=1e-6, cache=cache)
    block = MixLlamaMLP(gate_q, down_q, up_q, cache)
    norm.next_layer = block.up_proj_
    o = torch.nn.Linear(K, K, bias=True).half()            # (drawn after everything else: the three layers and the norm are what they were)
    o.weight.data.copy_(mkw(K, K))
    o.bias.data.copy_((0.1 * torch.randn(K, generator=g)).half())
    o_q = MixLinear_GEMM.from_linear(o.to(dtype), 8, weight_only=True, cache=cache, dev=dev)
    return torch.nn.ModuleList([norm, block, o_q])         # (one container: deepcopy keeps the cache shared between norm, block and layers)


def _forget(blk):
    """The twin keeps NOTHING between calls: whatever its layers derived (packed images, the padded / bf16 outlier operands, kept maps) goes
    through the product's one invalidation point and is rebuilt from the layer's state by the call that follows."""
    for m in blk.modules():
        if isinstance(m, MixLinear_GEMM):
            m._d.invalidate(weights=True, outliers=True)


NEW_RULES = ("forward_residual_contig", "forward_residual_3d", "forward_residual_strided", "layer_on_its_own_residual", "layer_on_its_own_o_proj",
             "o_proj_after_new_weights", "toggle_fuse_down_amax", "toggle_norm_kept_map")
NEW_RULES_BF16 = ("toggle_joint_gate_up_bf16",)
NEW_RULES_W4 = ("load_layer_outliers_both", "load_layer_outliers_weight_cache", "load_layer_outliers_realign")


class BlockMachine(RuleBasedStateMachine):
    BIT, K, I = 8, 128, 64
    DTYPE = torch.float16
    DEV, BACKEND = "cpu", backend_oracle                   # (tests/test_gpu_round6.py: "cuda" and the product's own HIP backend)
    FIRED = collections.Counter()                          # (class name, new rule) -> firings on a FROZEN block (both searches over)

    def __init__(self):
        super().__init__()
        self._prev = (swap_backend(L, self.BACKEND), swap_backend(F, self.BACKEND)) if self.BACKEND is not None else None
        self.a = self.b = None

    @classmethod
    def new_rules(cls):
        return NEW_RULES + (NEW_RULES_BF16 if cls.DTYPE == BF16 else ()) + (NEW_RULES_W4 if cls.BIT == 4 else ())

    def _frozen(self):
        blk = self.a[1]
        return not (blk.up_proj_.add_outliers or blk.down_proj_.add_outliers)

    def _fired(self, name):
        if self._frozen():
            BlockMachine.FIRED[(type(self).__name__, name)] += 1

    def _sync(self):
        if self.DEV != "cpu":
            torch.cuda.synchronize()

    def teardown(self):
        if self._prev is not None:
            swap_backend(L, self._prev[0])
            swap_backend(F, self._prev[1])

    @initialize(seed=st.integers(0, 3), warm=st.booleans())
    def build(self, seed, warm=False):
        """warm: the sequence starts where a serving process spends its life - three forwards in, both outlier searches over, the joint image
        and the kept plans built - instead of reaching that state by chance"""
        flags = BF16_FLAGS if self.DTYPE == BF16 else {}
        self.a = make_block(self.BIT, self.K, self.I, seed, MixqConfig(**flags), dev=self.DEV, dtype=self.DTYPE)   # every caching feature on (the defaults)
        self.b = make_block(self.BIT, self.K, self.I, seed, MixqConfig(**PLAIN, **flags), dev=self.DEV, dtype=self.DTYPE)   # the twin: nothing kept between forwards
        self.hot = [5, 77]
        self.step = 0
        self.new_weights = False                             # a checkpoint was loaded and the weight-only layer has not run since
        for i in range(3 if warm else 0):
            self.forward(16, i, False)

    # ---- what a serving process does ------------------------------------------------------------------------------------------------
    def _x(self, M, seed):
        x = torch.randn(M, self.K, generator=torch.Generator().manual_seed(1000 + seed)).to(self.DTYPE)
        x[:, self.hot] *= 30
        return x.to(self.DEV)

    def _residual(self, shape, kind, seed):
        """`kind`: "none"; "contig"; "3d" (3-D beside a 3-D x, else contiguous); "strided": rows 8 elements apart from the next one's start - a row
        stride that is a multiple of 4 and larger than out_features."""
        if kind == "none":
            return None
        N = shape[-1]
        wide = torch.randn(*shape[:-1], N + 8, generator=torch.Generator().manual_seed(3000 + seed)).to(self.DTYPE).to(self.DEV)
        return wide[..., :N] if kind == "strided" else wide[..., :N].contiguous()

    @rule(M=st.sampled_from([1, 3, 8, 16, 24]), seed=st.integers(0, 50), three_d=st.booleans(), res=st.sampled_from(["none", "contig", "3d", "strided"]))
    def forward(self, M, seed, three_d, res="none"):
        self.step += 1
        x = self._x(M, seed)
        if (three_d or res == "3d") and M % 2 == 0:
            x = x.reshape(2, M // 2, self.K)
        r = self._residual(tuple(x.shape), res, seed)
        if r is not None:
            self._fired("forward_residual_" + ("3d" if r.dim() == 3 else "strided" if res == "strided" else "contig"))
        if self.new_weights:
            self._fired("o_proj_after_new_weights")
            self.new_weights = False
        kw = {} if r is None else {"residual": r}            # (a call without it is the call it always was)
        _forget(self.b)
        ya = self.a[1](self.a[0](x.clone()), **kw)
        self._sync()                                         # (one per forward: a fault is reported at the step that caused it)
        yb = self.b[1](self.b[0](x.clone()), **kw)
        assert ya.shape == yb.shape and ya.dtype == yb.dtype == self.DTYPE and torch.equal(_bits(ya), _bits(yb)), \
            f"step {self.step}: block output differs from the cache-free twin's"
        oa, ob = self.a[2](ya, **kw), self.b[2](yb, **kw)     # the weight-only layer behind the block, on the same residual stream
        assert oa.shape == ob.shape and oa.dtype == ob.dtype == self.DTYPE and torch.equal(_bits(oa), _bits(ob)), \
            f"step {self.step}: the weight-only layer's output differs from the twin's"

    @rule(col=st.integers(0, 127))
    def new_hot_column(self, col):
        if col not in self.hot and len(self.hot) < 6:
            self.hot.append(col)

    @rule(M=st.sampled_from([2, 8, 16]), seed=st.integers(0, 50), which=st.sampled_from(["up_proj_", "down_proj_", "o_proj"]), residual=st.booleans())
    def layer_on_its_own(self, M, seed, which, residual=False):
        """o_proj-style direct call (unfused=True) of a layer that may have given its weights to the joint image, or of the weight-only layer
        (whose packed image is keyed on q_weight's identity and, in bfloat16, the dtype: it is also what runs first after new weights)"""
        la, lb = (self.a[2], self.b[2]) if which == "o_proj" else (getattr(self.a[1], which), getattr(self.b[1], which))
        x = torch.randn(M, la.in_features, generator=torch.Generator().manual_seed(2000 + seed)).to(self.DTYPE).to(self.DEV)
        r = self._residual((M, la.out_features), "contig" if residual else "none", seed)
        kw = {} if r is None else {"residual": r}
        if residual:
            self._fired("layer_on_its_own_residual")
        if which == "o_proj":
            self._fired("layer_on_its_own_o_proj")
            if self.new_weights:
                self._fired("o_proj_after_new_weights")
                self.new_weights = False
        _forget(self.b)
        ya, yb = la(x.clone(), None, True, **kw), lb(x.clone(), None, True, **kw)
        self._sync()
        assert ya.dtype == yb.dtype == self.DTYPE and torch.equal(_bits(ya), _bits(yb))

    @rule(seed=st.integers(0, 3))
    def load_new_weights(self, seed):
        """a checkpoint load into the live block (both blocks get the same tensors)"""
        flags = BF16_FLAGS if self.DTYPE == BF16 else {}
        src = make_block(self.BIT, self.K, self.I, 100 + seed, MixqConfig(**PLAIN, **flags), dev=self.DEV, dtype=self.DTYPE)
        sd = src.state_dict()
        self.new_weights = True
        # (a 4-bit layer that found new outlier columns has GROWN its registered `ind` / `weight_cache` buffers - linear.py:217-219 assigns the
        # hstack to the buffer names - and a fresh checkpoint no longer fits: the reference fails the same way; both blocks must agree)
        errs = []
        for blk in (self.a, self.b):
            try:
                blk.load_state_dict(copy.deepcopy(sd))
                errs.append(None)
            except RuntimeError as e:
                errs.append("size mismatch" in str(e))
        assert errs[0] == errs[1], errs
        if errs[0] is not None:                               # a refused load leaves both blocks as they were?  the next steps tell
            assert errs[0] is True

    @rule()
    def reload_own_state_dict(self):
        self.a.load_state_dict(self.a.state_dict())

    @rule()
    def half(self):
        self.a.half()                                         # (moves nothing: every tensor is fp16 / integer already)

    @rule()
    def deepcopy(self):
        self.a = copy.deepcopy(self.a)

    @rule()
    def toggle_joint_route(self):
        cfg = self.a[1].config
        cfg.joint_gate_up = not cfg.joint_gate_up

    @rule()
    def toggle_compaction_and_plans(self):
        cfg = self.a[1].config
        cfg.one_call_forward = not cfg.one_call_forward

    @precondition(lambda self: self.DTYPE != BF16)          # (the bfloat16 GEMMs have no nibble form: include/mixq_hip.h, "bf16 layers")
    @rule()
    def toggle_small_batch_image(self):
        """4-bit layers: a second, nibble image for batches of at most 8 rows (MixqConfig.small_batch_m4); nothing changes for 8-bit layers"""
        cfg = self.a[1].config
        cfg.small_batch_m4 = 0 if cfg.small_batch_m4 else 8

    @rule()
    def toggle_fuse_down_amax(self):
        """the row-maximum hand-over from the gate / joint GEMM to down_proj's quantiser, switched mid-life"""
        cfg = self.a[1].config
        cfg.fuse_down_amax = not cfg.fuse_down_amax
        self._fired("toggle_fuse_down_amax")

    @rule()
    def toggle_norm_kept_map(self):
        cfg = self.a[1].config
        cfg.norm_kept_map = not cfg.norm_kept_map
        self._fired("toggle_norm_kept_map")

    @precondition(lambda self: self.DTYPE == BF16)
    @rule()
    def toggle_joint_gate_up_bf16(self):
        cfg = self.a[1].config
        cfg.joint_gate_up_bf16 = not cfg.joint_gate_up_bf16
        self._fired("toggle_joint_gate_up_bf16")

    def random_step(self, rng):
        """One step drawn with a random.Random over the rules above and their arguments' ranges (tests/test_gpu_stateful.py: no hypothesis on
        the GPU, the sequence is readable from the seed); returns its description."""
        steps = [("forward", lambda: (rng.choice([1, 3, 8, 16, 24]), rng.randint(0, 50), rng.random() < 0.5, rng.choice(["none", "contig", "3d", "strided"]))),
                 ("new_hot_column", lambda: (rng.randint(0, 127),)),
                 ("layer_on_its_own", lambda: (rng.choice([2, 8, 16]), rng.randint(0, 50), rng.choice(["up_proj_", "down_proj_", "o_proj"]), rng.random() < 0.5)),
                 ("load_new_weights", lambda: (rng.randint(0, 3),)), ("reload_own_state_dict", tuple), ("half", tuple), ("deepcopy", tuple),
                 ("toggle_joint_route", tuple), ("toggle_compaction_and_plans", tuple), ("toggle_fuse_down_amax", tuple), ("toggle_norm_kept_map", tuple)]
        steps += [("toggle_joint_gate_up_bf16", tuple)] if self.DTYPE == BF16 else [("toggle_small_batch_image", tuple)]
        steps += [("load_layer_outliers", lambda: (rng.randint(0, 3), rng.choice(["both", "weight_cache", "realign"]), rng.random() < 0.5))] if self.BIT == 4 else []
        weights = [6 if name == "forward" else 1 for name, _ in steps]          # (a serving process mostly runs forwards)
        name, draw = rng.choices(steps, weights)[0]
        args = tuple(draw())
        getattr(self, name)(*args)
        self.same_reference_visible_state()
        self.no_bfloat16_in_the_state_dict()
        if self.step % 3 == 0:
            self.same_state_dict()
        return f"{name}{args}"

    @precondition(lambda self: self.BIT == 4)               # (8-bit layers: `ind` / `weight_cache` are runtime state, not in any state_dict)
    @rule(seed=st.integers(0, 3), what=st.sampled_from(["both", "weight_cache", "realign"]), between_forwards=st.booleans())
    def load_layer_outliers(self, seed, what, between_forwards=False):
        """a per-layer load_state_dict of `ind` / `weight_cache` into gate_proj_ ONLY, from a block with another hot set (its static columns; columns
        this block found online since are kept, so the sizes match): gate_proj then holds other columns than up_proj, which keeps the two
        launches (fused.py: _joint_applies) - or, "weight_cache": other values under the same `ind`, which the joint image's bf16 `wo` must
        follow.  "realign": up_proj's own `ind` / `weight_cache` into gate_proj - the joint image comes back.  between_forwards: the block runs right before and
        right after (the load meets images that were current - a joint image built from the tensors it changes), else the sequence decides."""
        if between_forwards:
            self.forward(16, seed, False)
        ga, gb = self.a[1].gate_proj_, self.b[1].gate_proj_
        if what == "realign":
            up = self.b[1].up_proj_
            sd = {"ind": up.ind.clone(), "weight_cache": up.weight_cache.clone()}
        else:
            flags = BF16_FLAGS if self.DTYPE == BF16 else {}
            g = make_block(self.BIT, self.K, self.I, 200 + seed, MixqConfig(**PLAIN, **flags), dev=self.DEV, dtype=self.DTYPE)[1].gate_proj_
            n0 = g.ind.shape[0]
            sd = {"weight_cache": torch.cat([g.weight_cache, gb.weight_cache[:, n0:]], dim=1)}
            if what == "both":
                sd["ind"] = torch.cat([g.ind, gb.ind[n0:]])
        assert all(tuple(sd[k].shape) == tuple(getattr(gb, k).shape) for k in sd)
        self._fired("load_layer_outliers_" + what)
        for gate in (ga, gb):
            gate.load_state_dict(copy.deepcopy(sd), strict=False)
        if between_forwards:
            self.forward(16, seed + 1, False)

    # ---- invariants --------------------------------------------------------------------------------------------------------------------
    @invariant()
    def same_reference_visible_state(self):
        if self.a is None:
            return
        for nm in ("up_proj_", "gate_proj_", "down_proj_"):
            la, lb = getattr(self.a[1], nm), getattr(self.b[1], nm)
            assert torch.equal(la.ind, lb.ind), nm
            assert la.cnt == lb.cnt and la.add_outliers == lb.add_outliers and la.forward_without_precondition_len == lb.forward_without_precondition_len, nm
            if lb.weight_cache is not None and lb.ind.numel():
                assert torch.equal(_bits(la.weight_cache), _bits(lb.weight_cache)), nm

    @precondition(lambda self: self.a is not None and self.step % 3 == 0)
    @invariant()
    def same_state_dict(self):
        sa, sb = self.a.state_dict(), self.b.state_dict()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(_bits(sa[k]), _bits(sb[k])), k

    @invariant()
    def no_bfloat16_in_the_state_dict(self):
        """the bf16 images (of weight_cache, of the joint image's wo) are derived and never saved"""
        if self.a is None or self.DTYPE != BF16:
            return
        for blk in (self.a, self.b):
            for k, v in blk.state_dict().items():
                assert v.dtype != BF16, k
                if k.endswith("weight_cache"):
                    assert v.dtype == torch.float16, k


class BlockMachine4(BlockMachine):
    BIT, K, I = 4, 256, 64


class BlockMachineBf16(BlockMachine):
    DTYPE = BF16


class BlockMachine4Bf16(BlockMachine4):
    DTYPE = BF16


_SETTINGS = settings(max_examples=60, stateful_step_count=24, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def assert_new_rules_fired(cls):
    """every rule this change added fired at least once on a FROZEN block during the run (derandomized: the counts are a fixed property)"""
    missing = [r for r in cls.new_rules() if not BlockMachine.FIRED[(cls.__name__, r)]]
    assert not missing, f"{cls.__name__}: never fired on a frozen block: {missing}"


def run_counted(cls, cfg=_SETTINGS):
    for key in [k for k in BlockMachine.FIRED if k[0] == cls.__name__]:
        del BlockMachine.FIRED[key]
    run_state_machine_as_test(cls, settings=cfg)
    assert_new_rules_fired(cls)
    return {r: BlockMachine.FIRED[(cls.__name__, r)] for r in cls.new_rules()}


class TestBlock8(BlockMachine.TestCase):
    settings = _SETTINGS

    def runTest(self):
        run_counted(BlockMachine, self.settings)
    runTest.is_hypothesis_test = True


class TestBlock4(BlockMachine4.TestCase):
    settings = _SETTINGS

    def runTest(self):
        run_counted(BlockMachine4, self.settings)
    runTest.is_hypothesis_test = True


def test_bf16_block_w8():
    print(run_counted(BlockMachineBf16))


def test_bf16_block_w4():
    print(run_counted(BlockMachine4Bf16))


def fixed_sequence(m):
    try:
        m.build(0)
        m.forward(16, 1, False); m.new_hot_column(9); m.forward(16, 2, True); m.forward(8, 3, False); m.forward(16, 4, False)
        assert m.a[1]._joint is not None and m.b[1]._joint is None            # the block under test took the joint route, the twin never does
        assert m.a[1].down_proj_._d.plan is not None and m.b[1].down_proj_._d.plan is None
        m.same_reference_visible_state(); m.same_state_dict()
        m.layer_on_its_own(8, 5, "up_proj_"); m.forward(16, 6, False)
        m.reload_own_state_dict(); m.forward(16, 7, False); m.deepcopy(); m.forward(24, 8, True)
        m.toggle_joint_route(); m.forward(16, 9, False); m.toggle_joint_route(); m.forward(16, 10, False)
        m.load_new_weights(1); m.forward(16, 11, False); m.half(); m.forward(3, 12, False)
        m.same_reference_visible_state(); m.same_state_dict()
    finally:
        m.teardown()


def fixed_sequence_ext(m):
    """The states this change is about, reached on purpose and ASSERTED to be reached (a test that cannot fail proves nothing): the joint
    route in the machine's dtype, a kept one-call plan that serves the same M with and without a residual, the route switches flipped on
    a frozen block, the weight-only layer re-packing after new weights and - 4-bit layers - gate_proj's differing columns forcing the two
    launches until they are realigned."""
    bf, w4 = m.DTYPE == BF16, m.BIT == 4
    try:
        m.build(0)
        blk, twin = m.a[1], m.b[1]
        if w4:
            m.hot = [int(c) for c in blk.up_proj_.ind[:2]]     # (hot columns among the static ones: no online growth, so checkpoints keep fitting)
        m.forward(16, 1, False); m.forward(16, 2, True, "3d"); m.forward(8, 3, False, "contig"); m.forward(16, 4, False)
        assert m._frozen()
        j = blk._joint
        assert j is not None and twin._joint is None and j["wo"] is not None and j["wo"].dtype == m.DTYPE        # the joint route ran, in this dtype
        assert not bf or blk.up_proj_._d.wpk is None                                                              # ... and holds the block's only image
        down = blk.down_proj_
        plan = down._d.plan
        assert plan is not None and plan.M == 16 and twin.down_proj_._d.plan is None
        assert getattr(plan, "dtype", m.DTYPE) == m.DTYPE
        for res in ("contig", "none", "strided", "none"):          # ONE kept plan serves this M with and without a residual
            m.forward(16, 5, False, res)
            assert down._d.plan is plan, res
        m.forward(16, 6, True, "3d")
        assert down._d.plan is plan
        m.toggle_fuse_down_amax(); m.forward(16, 7, False, "contig"); m.forward(16, 7, False); m.toggle_fuse_down_amax(); m.forward(16, 8, False, "strided")
        m.toggle_norm_kept_map(); m.forward(16, 9, False, "contig"); m.toggle_norm_kept_map(); m.forward(16, 10, False)
        if bf:
            m.toggle_joint_gate_up_bf16(); m.forward(16, 11, False, "contig")
            assert blk.up_proj_._d.wpk is not None and blk._joint is j          # the two launches, on images re-made from the joint one
            m.toggle_joint_gate_up_bf16(); m.forward(16, 12, False, "contig")
            assert blk.up_proj_._d.wpk is None                                  # ... released again by the joint route
        m.layer_on_its_own(8, 5, "up_proj_", True); m.forward(16, 13, False); m.layer_on_its_own(8, 6, "down_proj_", True); m.layer_on_its_own(8, 7, "o_proj", True)
        image = m.a[2]._d.wpk
        assert image is not None
        m.load_new_weights(1)
        assert m.new_weights
        m.layer_on_its_own(8, 8, "o_proj", False)
        assert m.a[2]._d.wpk is not image and not m.new_weights                 # the weight-only layer re-packed after new weights
        m.forward(16, 14, False, "strided")
        if w4:
            assert torch.equal(blk.up_proj_.ind, m.b[1].up_proj_.ind) and blk.up_proj_.ind.shape[0] == 32     # (the checkpoint did load)
            j = blk._joint
            m.load_layer_outliers(2, "both"); m.forward(16, 15, False, "contig")
            assert not torch.equal(blk.gate_proj_.ind, blk.up_proj_.ind)
            assert blk._joint is j and blk.up_proj_._d.wpk is not None          # gate_proj's differing columns: the two launches
            m.load_layer_outliers(0, "realign"); m.forward(16, 16, False, "contig")
            assert blk._joint is not j and blk._joint["key"] == blk._joint_key() and blk.up_proj_._d.wpk is None     # the joint image came back
            assert blk._joint["wo"].dtype == m.DTYPE
            j = blk._joint
            m.load_layer_outliers(3, "weight_cache"); m.forward(16, 17, False)
            assert blk._joint is not j                                          # other values under the same `ind`: the image followed
        m.same_reference_visible_state(); m.same_state_dict(); m.no_bfloat16_in_the_state_dict()
        m.deepcopy(); m.forward(24, 18, True, "3d"); m.half(); m.forward(3, 19, False, "contig"); m.reload_own_state_dict(); m.forward(16, 20, False, "strided")
        m.same_reference_visible_state(); m.same_state_dict(); m.no_bfloat16_in_the_state_dict()
    finally:
        m.teardown()


def test_fixed_sequence_on_the_oracle_backend():
    """One hand-written sequence through the same machine (what tests/test_gpu_round6.py replays on the GPU): search, a new column, freeze,
    joint route, a direct layer call, state_dict round trip, deepcopy, new weights."""
    fixed_sequence(BlockMachine())
    fixed_sequence(BlockMachine4())


MACHINES = [BlockMachine, BlockMachine4, BlockMachineBf16, BlockMachine4Bf16]


@pytest.mark.parametrize("cls", MACHINES, ids=lambda c: c.__name__)
def test_fixed_sequences_on_every_machine(cls):
    """fixed_sequence on the bfloat16 machines too, and fixed_sequence_ext - whose asserts say which states were reached - on all four
    (tests/test_gpu_stateful.py replays both on the GPU)."""
    if cls.DTYPE == BF16:
        fixed_sequence(cls())
    fixed_sequence_ext(cls())


# ---- wrong products: each must make a machine raise within its derandomized budget ---------------------------------------------------------
_NO_SHRINK = settings(_SETTINGS, phases=[Phase.generate])    # (the same examples; a failure is reported as found, not minimised)


def _stale_wo_operand(self):
    """(a) `_wo_operand` whose key ignores `_version` / identity: the bf16 image of weight_cache outlives a load / new values"""
    wc, dt = self.weight_cache, self.act_dtype
    key = (tuple(wc.shape), wc.stride(0), dt)
    if self._wo_key != key:
        self._wo_ready, self._wo_key = L._gemm_ready(wc if wc.dtype == dt else wc.to(dt)), key
    return self._wo_ready


def _plan_run_dropping_addend(run):
    """(b) the one-call route loses the residual (the twin's two-call route does not)"""
    def wrong(self, x, row_amax=None, col_mask=None, addend=None):
        return run(self, x, row_amax=row_amax, col_mask=col_mask)
    return wrong


def _forward_with_a_sticky_pack_key(forward):
    """(c) the weight-only pack key without q_weight's identity / `_version`: once packed, the image is taken for current"""
    def wrong(self, x, *args, **kw):
        if self.weight_only and self._wpk is not None:
            qw = self.q_weight
            self._wpk_key = (id(qw), qw.data_ptr(), qw._version) + ((self.act_dtype,) if self.act_dtype != torch.float16 else ())
        return forward(self, x, *args, **kw)
    return wrong


def _joint_key_without_weight_cache(self):
    """(d) `_joint_key` without ident(l.weight_cache)"""
    up, gate = self.up_proj_, self.gate_proj_

    def ident(t):
        return None if t is None else (id(t), t._version, tuple(t.shape))
    return tuple((ident(l._buffers.get("q_weight")), ident(l.scale_col), ident(l.bias), ident(l.ind)) for l in (up, gate)) + (str(up.scale_col.device),) + self.config.key()


WRONG = {"stale_wo_operand": (BlockMachine4Bf16, MixLinear_GEMM, "_wo_operand", lambda old: _stale_wo_operand),
         "plan_drops_addend": (BlockMachineBf16, backend_oracle.ForwardPlan, "run", _plan_run_dropping_addend),
         "sticky_w8a16_pack_key": (BlockMachineBf16, MixLinear_GEMM, "forward", _forward_with_a_sticky_pack_key),
         "joint_key_without_weight_cache": (BlockMachine4Bf16, MixLlamaMLP, "_joint_key", lambda old: _joint_key_without_weight_cache)}


@pytest.mark.parametrize("name", list(WRONG))
def test_a_wrong_product_makes_the_machine_raise(name, monkeypatch):
    cls, owner, attr, make = WRONG[name]
    monkeypatch.setattr(owner, attr, make(getattr(owner, attr)))
    with pytest.raises(AssertionError):
        run_state_machine_as_test(cls, settings=_NO_SHRINK)
