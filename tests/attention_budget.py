"""Error budget of the pointwise attention: a float64 truth, the fp32 reference's own loss on the same case as the yardstick, and a
gate at a small multiple of it -- per piece, never per whole tensor.

Reference.  For one case (weights w, candidates t, history h, upstream gradient g; fp32 values) the CPU oracle's literal
[B,T,H,4D]-concat attention runs twice: in float64 (R64, the truth) and in float32 (R32, the reference's own arithmetic).  For the
fused attention + pool node the output is pooled = einsum(s, h) and g is the pooled gradient.

Pieces.  s / pooled, d_target, d_history: one piece per impression b, the figure of the tensor is its worst impression.  The
fc1.weight gradient: its four [D, D] column blocks [W_h | W_t | W_d | W_p] (they come from different kernels).  fc1.bias, fc2.weight,
fc2.bias gradients: whole.  Two norms per piece: max|got - R64| / max|R64| and ||got - R64|| / ||R64||.  A piece whose float64
reference is all zero is an error of the case, not a pass (``_piece_err`` asserts).

Yardstick and gate.  Y(piece, norm) = max(err(R32 against R64), 2**-23): what the reference's own arithmetic loses on this very
case, floored at one fp32 unit roundoff of the piece's scale.  A result passes when err(result against R64) <= M * Y for every
piece and both norms; M depends on the arithmetic only.  For bf16x3 the yardstick is Y3 = max(err(E3 against R64), Y) with E3 the CPU
emulation below ("is this bf16x3", not "how far is bf16x3 from fp32").

M_F32 / M_BF16X3: the smallest power of two >= 4 x the worst ratio any kernel form reached in the recorded MI355X run of
tests/test_gpu_attention_budget.py, profiles/attention_error_budget.json (worst ratios and the rule are repeated there and in
DESIGN.md).  Condition on both, checked by tests/test_attention_budget_cpu.py: every mutant below is still rejected at 4 * M."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import user_model_oracle as orc

# profiles/attention_error_budget.json (one MI355X run of tests/test_gpu_attention_budget.py): the worst ratio of any piece but
# d_fc2.bias is 4.2 for f32 (d_history, dP walk, (1,64,128,768)) and 2.6 for bf16x3 (d_fc2.weight, (3,7,19,72), family small).
M_F32 = 32
M_BF16X3 = 16
# The fc2.bias gradient is sum(ds) over all B*T*H scores, formed on the device in fp32 (partial sums, then float atomics) in both
# arithmetics.  The CPU's fp32 sum is right to 1e-8, so the piece is judged against the 2**-23 floor -- relative to the RESULT, while
# the roundings are relative to the partial sums, and a sum of N(0,1) entries cancels: recorded worst 10.6 floors (bf16x3,
# (3,5,130,208); f32 8.9 at (2,20,10,256)), where sum|g| / |sum g| is 236 and 185 and a sequential fp32 sum on the CPU is 40 and 9
# floors off; no form stands out.  Explained by the arithmetic, so the piece has its own constant by the same rule; a row lost
# from this sum (mutant drop_row) measures > 1e4 floors in this piece alone.
M_FC2_BIAS = 64
M = {"f32": M_F32, "bf16x3": M_BF16X3}
PIECE_M = {"d_fc2.bias": M_FC2_BIAS}


def m_of(piece, arithmetic):
    return PIECE_M.get(piece, M[arithmetic])


FLOOR = 2.0 ** -23
WKEYS = ("mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
FAMILIES = ("normal", "x8", "small", "mixed", "dup", "padded", "bf16_exact")
MUTANTS = ("tanh_gelu", "gelu_grad_at_bf16_z", "drop_cross_term", "drop_row", "drop_last_history_row_of_dv", "stale_block")

# per-launch knobs of the fp32 attention (read at every launch): forward image / walk forms and every backward form
FORMS = {
    "default": {},
    "fwd_ct0": {"NRM_FWD_CT": "0"},
    "fwd_ct1": {"NRM_FWD_CT": "1"},
    "walk_f32_0": {"NRM_FWD_WALK_F32": "0"},
    "walk_f32_1": {"NRM_FWD_WALK_F32": "1"},
    "e_form": {"NRM_BWD_DP": "0"},
    "dp_walk": {"NRM_BWD_DP": "1"},
    "dp_walk_grid1": {"NRM_BWD_DP": "1", "NRM_DP_GRID": "1"},
    "dz_rows0": {"NRM_DZ_ROWS": "0"},
    "dz_rows1": {"NRM_DZ_ROWS": "1"},
}


def form_skip_reason(form, D, H, lib):
    """Why a form of FORMS says nothing at this shape (None: it applies)."""
    if form.startswith("walk") and D not in (64, 128):
        return "the fp32 walk switch only matters at D = 64 / 128"
    if form.startswith("fwd_ct") and (D <= 128 or D % 4):
        return "the candidate-image switch only matters for the chunk-streaming fp32 forward"
    if form.startswith("dp_") and not lib.nrm_pwattn_bwd_dp_supported(D, H):
        return "no dP walk for this shape"
    return None


# ------------------------------------------------------------------------------------------------ cases
def weights(rng, D):
    k1, k2 = 1 / np.sqrt(4 * D), 1 / np.sqrt(D)
    return {"mlp.fc1.weight": rng.uniform(-k1, k1, (D, 4 * D)).astype(np.float32),
            "mlp.fc1.bias": rng.uniform(-k1, k1, (D,)).astype(np.float32),
            "mlp.fc2.weight": rng.uniform(-k2, k2, (1, D)).astype(np.float32),
            "mlp.fc2.bias": rng.uniform(-k2, k2, (1,)).astype(np.float32)}


def _to_bf16(a):
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


class Case:
    """One set of inputs with its cached references and yardsticks."""

    def __init__(self, w, t, h, g, pool=False, tag=None):
        self.w = {k: np.ascontiguousarray(w[k], dtype=np.float32) for k in WKEYS}
        self.t, self.h, self.g = (np.ascontiguousarray(x, dtype=np.float32) for x in (t, h, g))
        self.pool = bool(pool)
        self.out = "pooled" if pool else "s"
        self.B, self.T, self.D = self.t.shape
        self.H = self.h.shape[1]
        assert self.g.shape == ((self.B, self.T, self.D) if pool else (self.B, self.T, self.H))
        self.tag = tag or {}
        self._cache = {}

    def reference(self, dtype):
        """The oracle's result in ``dtype`` (torch.float64: R64, torch.float32: R32) as float64 numpy arrays."""
        key = ("ref", dtype)
        if key not in self._cache:
            p = {"a." + k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in self.w.items()}
            t = torch.from_numpy(self.t).to(dtype).requires_grad_(True)
            h = torch.from_numpy(self.h).to(dtype).requires_grad_(True)
            out = orc.pointwise_attention_scores(p, "a", t, h)[..., 0]
            if self.pool:
                out = torch.einsum("bth,bhd->btd", out, h)
            (out * torch.from_numpy(self.g).to(dtype)).sum().backward()
            res = {self.out: out.detach(), "d_target": t.grad, "d_history": h.grad}
            res.update({k: p["a." + k].grad for k in WKEYS})
            self._cache[key] = {k: v.double().numpy() for k, v in res.items()}
        return self._cache[key]

    def yardstick(self, arithmetic, order=0):
        """{(piece, norm): Y}; for bf16x3 Y3 from the emulation evaluated in ``order``."""
        key = ("Y", arithmetic, order)
        if key not in self._cache:
            r64 = self.reference(torch.float64)
            y = {k: max(v, FLOOR) for k, v in errors(self.reference(torch.float32), r64, self.D).items()}
            if arithmetic == "bf16x3":
                e3 = errors(emulate(self, "bf16x3", order=order), r64, self.D)
                y = {k: max(v, e3[k]) for k, v in y.items()}
            elif arithmetic != "f32":
                raise ValueError(f"no budget for arithmetic {arithmetic!r} (plain bf16 is characterised, not gated)")
            self._cache[key] = y
        return self._cache[key]


def make_inputs(B, T, H, D, family="normal", seed=None, pool=False):
    """Seeded (w, t, h, g) of one input family.  ``normal`` with the default seed is what the attention tests have always built.
    Two families degenerate where a piece's reference would otherwise be exactly zero: ``dup`` leaves impression 0 alone when
    T = H = 1 (so at B = 1 it IS ``normal``: ``family_is_degenerate``), ``padded`` keeps a lone candidate (T = 1) non-zero and
    zeroes no history row when H < 3."""
    rng = np.random.default_rng(B * 1000 + T * 100 + H * 10 + D if seed is None else seed)
    w = weights(rng, D)
    t = rng.standard_normal((B, T, D)).astype(np.float32)
    h = rng.standard_normal((B, H, D)).astype(np.float32)
    g = rng.standard_normal((B, T, D) if pool else (B, T, H)).astype(np.float32)
    if family == "normal":
        pass
    elif family == "x8":                         # most pre-activations in the GELU tails, exp(-z^2 / 2) underflows
        t, h = t * np.float32(8), h * np.float32(8)
    elif family == "small":                      # GELU near its linear part
        t, h = t * np.float32(1e-3), h * np.float32(1e-3)
    elif family == "mixed":                      # impression b scaled by 2**k_b, k_b in [-6, 3]; a loud first and a quiet last one
        k = rng.integers(-6, 4, size=B)
        k[0] = 3
        if B > 1:
            k[-1] = -6
        sc = (2.0 ** k).astype(np.float32)[:, None, None]
        t, h = t * sc, h * sc
    elif family == "dup":                        # a candidate that equals a history row: the reference forms t - h = 0 exactly
        n = min(T, H)
        b0 = 1 if T == 1 and H == 1 else 0       # (one pair per impression: the first keeps t != h, or the W_d gradient block would be exactly 0)
        h[b0:, :n] = t[b0:, :n]
    elif family == "padded":                     # all-zero padding rows are scored, not masked; g stays non-zero everywhere
        if H // 3:
            h[:, H - H // 3:] = 0.0
        if T > 1:                                # (a lone candidate stays: with t = 0 the W_t and W_p gradient blocks would be exactly 0)
            t[:, T - 1] = 0.0
    elif family == "bf16_exact":                 # every lo operand of the weights and side projections is zero
        t, h = _to_bf16(t), _to_bf16(h)
        w = {k: _to_bf16(v) for k, v in w.items()}
    else:
        raise ValueError(family)
    return w, t, h, g


def family_is_degenerate(shape, family):
    """True where the family's construction leaves the inputs of ``normal`` unchanged (callers drop such cases: they test nothing new)."""
    B, T, H, D = shape
    return (family == "dup" and B == 1 and T == 1 and H == 1) or (family == "padded" and T == 1 and H < 3)


_cases = {}


def get_case(shape, family="normal", seed=None, pool=False):
    """Cached Case: many kernel forms share one case (and its two oracle passes)."""
    key = (tuple(shape), family, seed, bool(pool))
    if key not in _cases:
        if len(_cases) >= 48:                    # bounded: the big cases hold a few hundred MB of float64 references
            _cases.pop(next(iter(_cases)))
        B, T, H, D = shape
        _cases[key] = Case(*make_inputs(B, T, H, D, family, seed, pool), pool=pool,
                           tag={"shape": list(shape), "family": family})
    return _cases[key]


# ------------------------------------------------------------------------------------------------ pieces, errors, gate
BLOCKS = ("W_h", "W_t", "W_d", "W_p")


def pieces(name, a, D):
    """{piece name: [arrays]} of one tensor; the figure of a piece is the worst of its arrays."""
    if name in ("s", "pooled", "d_target", "d_history"):
        return {name: [a[b] for b in range(a.shape[0])]}
    if name == "mlp.fc1.weight":
        return {f"d_fc1.weight[{BLOCKS[i]}]": [a[:, i * D:(i + 1) * D]] for i in range(4)}
    return {"d_" + name[4:]: [a]}


def _piece_err(name, got, ref):
    mx = l2 = 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        assert g.shape == r.shape, (name, i, g.shape, r.shape)
        den_mx, den_l2 = np.abs(r).max(), np.linalg.norm(r)
        assert den_mx > 0 and den_l2 > 0 and np.isfinite(den_l2), f"piece {name}[{i}]: the float64 reference is zero or non-finite"
        d = g - r
        e_mx, e_l2 = np.abs(d).max() / den_mx, np.linalg.norm(d) / den_l2
        if not (np.isfinite(e_mx) and np.isfinite(e_l2)):
            e_mx = e_l2 = float("inf")
        mx, l2 = max(mx, float(e_mx)), max(l2, float(e_l2))
    return mx, l2


def errors(got, ref, D, rowgrads=True):
    """{(piece, norm): error of got against ref} over EVERY piece of ref (minus the two row gradients when ``rowgrads`` is False:
    the weight-only backward does not form them, and then got must not carry them either)."""
    skip = () if rowgrads else ("d_target", "d_history")
    if not rowgrads:
        assert not any(k in got for k in skip), "row gradients given to a weight-only check"
    out = {}
    for k in ref:
        if k in skip:
            continue
        assert k in got, f"missing result {k!r}"
        pg, pr = pieces(k, np.asarray(got[k]).reshape(np.shape(ref[k])), D), pieces(k, ref[k], D)
        for name in pr:
            mx, l2 = _piece_err(name, pg[name], pr[name])
            out[(name, "max")], out[(name, "l2")] = mx, l2
    return out


def ratios(got, case, arithmetic, rowgrads=True, order=0):
    """{(piece, norm): err(got against R64) / Y}."""
    y = case.yardstick(arithmetic, order)
    e = errors(got, case.reference(torch.float64), case.D, rowgrads)
    return {k: v / y[k] for k, v in e.items()}


def assert_within_budget(got, case, arithmetic, rowgrads=True, order=0, m=None, record=None, **tag):
    """``got``: {'s' | 'pooled', 'd_target', 'd_history', the four weight names: arrays}.  Raises with the piece, norm, measured ratio
    and M when any piece is over budget; returns all ratios.  ``record``: a list that receives one entry per ratio."""
    r = ratios(got, case, arithmetic, rowgrads, order)
    if record is not None:
        meta = dict(case.tag, entry="attend_and_pool" if case.pool else "scores", arithmetic=arithmetic, **tag)
        record.extend(dict(meta, piece=p, norm=n, ratio=float(v)) for (p, n), v in r.items())
    lim = (lambda piece: m_of(piece, arithmetic)) if m is None else (lambda piece: m)
    over = {k: v for k, v in r.items() if not v <= lim(k[0])}
    if over:
        (piece, norm), w = max(over.items(), key=lambda kv: kv[1] / lim(kv[0][0]))
        raise AssertionError(f"over the {arithmetic} error budget: piece {piece}, norm {norm}: {w:.1f} x the yardstick "
                             f"(M = {lim(piece)}); all pieces over: " + ", ".join(f"{p}/{n} {v:.1f}" for (p, n), v in sorted(over.items())))
    return r


def worst(r):
    return max(r.values())


def worst_margin(r, arithmetic):
    """((piece, norm), ratio, ratio / M of that piece) of the entry that is furthest out in units of its own constant."""
    k = max(r, key=lambda k: r[k] / m_of(k[0], arithmetic))
    return k, r[k], r[k] / m_of(k[0], arithmetic)


def from_run_both(s, got):
    """The (scores, grads) pair of tests/test_gpu_attention.py's _run_both in the names used here."""
    out = {"s": s, "d_target": got["target"], "d_history": got["history"]}
    out.update({k: got[k] for k in WKEYS})
    return out


def run_device(case, mma, rowgrads=True):
    """The case through ops.pointwise_attention_scores / ops.attend_and_pool and autograd on the GPU -> result dict."""
    from news_recommendation_model_amd import ops
    wg = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in case.w.items()}
    t = torch.from_numpy(case.t).cuda().requires_grad_(rowgrads)
    h = torch.from_numpy(case.h).cuda().requires_grad_(rowgrads)
    fn = ops.attend_and_pool if case.pool else ops.pointwise_attention_scores
    out = fn(t, h, *(wg[k] for k in WKEYS), mma=mma)
    (out * torch.from_numpy(case.g).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {case.out: out.detach().cpu().numpy()}
    if rowgrads:
        got.update(d_target=t.grad.cpu().numpy(), d_history=h.grad.cpu().numpy())
    got.update({k: wg[k].grad.cpu().numpy() for k in WKEYS})
    return got


def write_record(path, entries):
    """One JSON file: the constants, the worst ratio per arithmetic (d_fc2.bias apart, see M_FC2_BIAS) and per piece with the case
    that produced it, and every ratio grouped by run (entry, arithmetic, form, shape, family -> {"piece|norm": ratio})."""
    def where(e):
        return {k: e[k] for k in ("ratio", "piece", "norm", "entry", "form", "shape", "family")}

    gated = [e for e in entries if e["arithmetic"] in M]
    summary = {"M": dict(M, **PIECE_M), "worst_ratio": {}, "worst_per_piece": {},
               "rule": "M = the smallest power of two >= 4 x the worst recorded ratio; d_fc2.bias (float-atomic sum of all ds, judged "
                       "against the 2**-23 floor) has its own constant by the same rule"}
    for arith in M:
        rest = [e for e in gated if e["arithmetic"] == arith and e["piece"] not in PIECE_M]
        if rest:
            summary["worst_ratio"][arith] = where(max(rest, key=lambda e: e["ratio"]))
        for piece in sorted({e["piece"] for e in gated if e["arithmetic"] == arith}):
            es = [e for e in gated if e["arithmetic"] == arith and e["piece"] == piece]
            summary["worst_per_piece"][f"{arith}|{piece}"] = where(max(es, key=lambda e: e["ratio"]))
    for piece in PIECE_M:
        es = [e for e in gated if e["piece"] == piece]
        if es:
            summary["worst_ratio"][piece] = dict(where(max(es, key=lambda e: e["ratio"])), arithmetic=max(es, key=lambda e: e["ratio"])["arithmetic"])
    runs = {}
    for e in entries:
        key = (e["entry"], e["arithmetic"], e["form"], tuple(e["shape"]), e["family"], e.get("rowgrads_wanted", True))
        runs.setdefault(key, {})[e["piece"] + "|" + e["norm"]] = float(f"{e['ratio']:.4g}")
    summary["runs"] = [dict(entry=k[0], arithmetic=k[1], form=k[2], shape=list(k[3]), family=k[4], rowgrads=k[5], ratios=v)
                       for k, v in runs.items()]
    runs = summary.pop("runs")
    with open(path, "w") as f:                             # one run per line: a later recording diffs run by run
        f.write(json.dumps(summary, indent=1)[:-2] + ',\n "runs": [\n')
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in runs))
        f.write("\n ]\n}\n")


def record_path():
    return os.environ.get("NRM_BUDGET_RECORD") or None


# ------------------------------------------------------------------------------------------------ CPU emulations
def _split(x):
    hi = x.to(torch.bfloat16).to(torch.float32)
    return hi, (x - hi).to(torch.bfloat16).to(torch.float32)


def _mm(a, b, order):
    """fp32 a @ b; order 1: the transposed product with the reduction split in two halves (another summation order)."""
    if order == 0:
        return a @ b
    k = a.shape[1] // 2
    if k == 0:
        return (b.t() @ a.t()).t()
    return ((b[:k].t() @ a[:, :k].t()) + (b[k:].t() @ a[:, k:].t())).t()


def _product(a, b, mode, order):
    """a @ b as the matrix cores form it.  mode 0: fp32; 3: bf16x3 = hi*hi + hi*lo + lo*hi of bf16-split operands, fp32
    accumulation; 2: the lo*hi cross term dropped (a mutant); 1: plain bf16 = hi*hi."""
    if mode == 0:
        return _mm(a, b, order)
    ah, al = _split(a)
    bh, bl = _split(b)
    r = _mm(ah, bh, order)
    if mode >= 2:
        r = r + _mm(ah, bl, order)
    if mode >= 3:
        r = r + _mm(al, bh, order)
    return r


class _Product(torch.autograd.Function):
    """a @ b with every product of the forward AND of the backward (g b^T, a^T g: the transposed forms, du^T h, dv^T t, dP = dz W_p,
    the dW_p sum) in the given arithmetic.  The incoming gradient (dz, du, dv) is split into bf16 hi/lo for EVERY shape, which is what
    the hi/lo dz storage of the resident-W backward holds (nrm_pwattn_bwd_rw_supported: D <= 256); the wider bf16 forms split the fp32
    dz at operand read instead, into the same hi/lo pair and the same three products, so the emulation takes no condition on the
    shape -- and needs no library, which keeps it usable where there is no GPU build.  Recorded device results sit at 0.8 .. 1.6 Y3
    on both sides of D = 256 (profiles/attention_error_budget.json)."""

    @staticmethod
    def forward(ctx, a, b, mode, order):
        ctx.save_for_backward(a, b)
        ctx.mode, ctx.order = mode, order
        return _product(a, b, mode, order)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _product(g, b.t(), ctx.mode, ctx.order), _product(a.t(), g, ctx.mode, ctx.order), None, None


_MODES = {"f32": 0, "bf16": 1, "bf16x3": 3}


def median_grad_row(g):
    """Index (b, t, h) of the upstream-gradient entry whose |g| is the median."""
    a = np.abs(g).reshape(-1)
    return np.unravel_index(int(np.argsort(a, kind="stable")[a.size // 2]), g.shape)


def emulate(case, arithmetic, mutant=None, order=0):
    """torch-CPU fp32 evaluation in the kernels' association, z = h (W_h - W_d)^T + b1 + t (W_t + W_d)^T + (t*h) W_p^T,
    s = w2 . gelu(z) + b2, and its autograd; for bf16x3 / bf16 every product ops.py sends to the bf16 matrix cores (the
    contraction, both side projections and all their backward forms) is emulated by _Product.  ``mutant``: one of MUTANTS."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    if mutant == "drop_cross_term" and arithmetic != "bf16x3":
        raise ValueError("drop_cross_term is a mutant of bf16x3")
    if mutant == "drop_row" and case.pool:
        raise ValueError("drop_row is defined on the scores entry")
    key = ("emu", arithmetic, mutant, order)
    if key in case._cache:
        return case._cache[key]
    mode = 2 if mutant == "drop_cross_term" else _MODES[arithmetic]
    B, T, H, D = case.B, case.T, case.H, case.D

    def run(g_np):
        p = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in case.w.items()}
        t = torch.from_numpy(case.t).clone().requires_grad_(True)
        h = torch.from_numpy(case.h).clone().requires_grad_(True)
        w1 = p["mlp.fc1.weight"]
        wh, wt, wd, wp = (w1[:, i * D:(i + 1) * D] for i in range(4))
        u = _Product.apply(h.reshape(B * H, D), (wh - wd).t(), mode, order).reshape(B, H, D) + p["mlp.fc1.bias"]
        v = _Product.apply(t.reshape(B * T, D), (wt + wd).t(), mode, order).reshape(B, T, D)
        vb = v[:, :, None, :].expand(B, T, H, D)
        if mutant == "drop_last_history_row_of_dv":        # same values; the sum over h behind dv misses h = H-1 of the last impression
            keep = torch.ones(B, 1, H, 1)
            keep[B - 1, 0, H - 1, 0] = 0.0
            vb = vb * keep + (vb * (1.0 - keep)).detach()
        prod = (t[:, :, None, :] * h[:, None, :, :]).reshape(B * T * H, D)
        z = _Product.apply(prod, wp.t(), mode, order).reshape(B, T, H, D) + u[:, None] + vb
        if mutant == "tanh_gelu":
            a = F.gelu(z, approximate="tanh")
        elif mutant == "gelu_grad_at_bf16_z":              # the value from the fp32 z, the derivative from a bf16-rounded copy
            zr = z.detach().to(torch.bfloat16).float().requires_grad_(True)
            (gp,) = torch.autograd.grad(F.gelu(zr).sum(), zr)
            a = F.gelu(z).detach() + (z - z.detach()) * gp
        else:
            a = F.gelu(z)
        s = (a * p["mlp.fc2.weight"].reshape(-1)).sum(-1) + p["mlp.fc2.bias"]
        out = torch.einsum("bth,bhd->btd", s, h) if case.pool else s
        (out * torch.from_numpy(g_np)).sum().backward()
        res = {case.out: out.detach(), "d_target": t.grad, "d_history": h.grad}
        res.update({k: p[k].grad for k in WKEYS})
        return {k: v.double().numpy() for k, v in res.items()}

    res = run(case.g)
    if mutant == "drop_row":                               # the weight-gradient sums miss one (b,t,h) row; row gradients untouched
        g2 = case.g.copy()
        g2[median_grad_row(case.g)] = 0.0
        res.update({k: v for k, v in run(g2).items() if k in WKEYS})
    if mutant == "stale_block":                            # the W_d block taken as da_t alone instead of da_t - da_h
        w1g = res["mlp.fc1.weight"].copy()
        w1g[:, 2 * D:3 * D] = w1g[:, D:2 * D]
        res["mlp.fc1.weight"] = w1g
    case._cache[key] = res
    return res
