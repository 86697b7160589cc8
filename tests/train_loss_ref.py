"""Restatements of the three entry points of csrc/lz_train.hip, for the tests only (numpy and torch on the CPU).

`ref_loss`: the fused policy + bucketed-value loss in float64.  Only the scalar chain that assigns the value bins is
taken in float32, expression by expression as oracle/loss_oracle.py:47-63 has it (draw test, anti-draw substitution,
mixed, u, lo, hi, frac): that chain is the specification of the bin assignment, not rounding.  Everything else --
combined logits, the masked log-sum-exp, the -50 replacement and clamp, CE - H, the value log-softmax, the WDL term
with its empty draw class, every sum -- is float64.  The gradients are produced twice: by float64 autograd on the
forward restatement, and written out by hand (dL/d combined, then the scatter onto lp1 / lp2 / lpm); `ref_loss`
asserts that the two agree to 1e-12, so the tests do not rest on one derivation.

`ref_pack` / `ref_unpack`: plain per-row loops over the record layout that include/liuzhou_hip.h documents.
tests/test_train_loss_ref_cpu.py anchors all of it (g11 / g21 fixtures, the fp32 oracle, literal records)."""
import numpy as np
import torch

BINS = 101
TOTAL = 220
RECORD_BYTES = 360
POLICY_SLOTS = 72
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))                 # up, down, left, right


def move_dest(frm, d):
    """Destination cell of the move `d` from cell `frm`, or -1 off the board."""
    r, c = divmod(frm, 6)
    nr, nc = r + DIRS[d][0], c + DIRS[d][1]
    return nr * 6 + nc if 0 <= nr < 6 and 0 <= nc < 6 else -1


MOVE_FROM = np.repeat(np.arange(36), 4)
MOVE_DEST = np.array([move_dest(f, d) for f in range(36) for d in range(4)])
ON_BOARD = MOVE_DEST >= 0


def value_bins_fp32(value, soft, alpha, anti_draw):
    """The float32 scalar chain of oracle/loss_oracle.py:47-63 -> draw (bool), mixed, lo, hi, frac (torch, CPU)."""
    raw = torch.as_tensor(value, dtype=torch.float32).reshape(-1)
    soft = torch.as_tensor(soft, dtype=torch.float32).reshape(-1)
    draw = raw.abs() < 1e-8
    v = raw.clone()
    if abs(float(anti_draw)) > 1e-9:
        v[draw] = float(anti_draw)
    a = float(max(0.0, min(1.0, alpha)))
    mixed = ((1.0 - a) * v + a * soft).clamp(-1.0, 1.0)
    step = 2.0 / (BINS - 1)
    u = (mixed + 1.0) / step
    lo = torch.floor(u).long().clamp(0, BINS - 1)
    hi = (lo + 1).clamp(0, BINS - 1)
    frac = (u - lo.float()).clamp(0.0, 1.0)
    frac = torch.where(hi == lo, torch.zeros_like(frac), frac)
    return draw, mixed, lo, hi, frac


def _combined(lp1, lp2, lpm):
    B = lp1.shape[0]
    dest = torch.from_numpy(np.where(ON_BOARD, MOVE_DEST, 0))
    moves = lp2[:, torch.from_numpy(MOVE_FROM)] + lp1[:, dest]
    moves = torch.where(torch.from_numpy(ON_BOARD).expand(B, -1), moves, torch.full_like(moves, float("-inf")))
    return torch.cat([lp1, moves, lpm, torch.zeros((B, 4), dtype=lp1.dtype)], dim=1)


def _policy_forward(comb, legal, target):
    """-> kl [B], log-probabilities [B,220], softmax over the live entries [B,220], live, lse_ok."""
    live = legal & torch.isfinite(comb)                   # the entries that take part in the log-sum-exp
    lse_ok = live.any(dim=1, keepdim=True)                # == has-legal and finite lse: heads are <= 0 or -inf
    safe = torch.where(live, comb, torch.zeros_like(comb))
    mx = torch.where(live, comb, torch.full_like(comb, float("-inf"))).amax(dim=1, keepdim=True).detach()
    mx = torch.where(lse_ok, mx, torch.zeros_like(mx))
    ex = torch.where(live, torch.exp(safe - mx), torch.zeros_like(comb))
    se = ex.sum(dim=1, keepdim=True)
    lse = torch.where(lse_ok, mx + torch.log(torch.where(lse_ok, se, torch.ones_like(se))), torch.zeros_like(mx))
    lp = torch.where(live, safe - lse, torch.full_like(comb, -50.0))         # legal but -inf: replaced by -50, no gradient
    lp = torch.where(legal, lp, torch.zeros_like(comb))
    ce = -(target * lp.clamp(min=-50.0)).sum(dim=1)
    ent = -(target * target.clamp(min=1e-8).log()).sum(dim=1)
    p = torch.where(lse_ok, ex / torch.where(lse_ok, se, torch.ones_like(se)), torch.zeros_like(ex))
    return ce - ent, lp, p, live, lse_ok


def ref_loss(lp1, lp2, lpm, vlogits, legal, target, value, soft, *, alpha, anti_draw, draw_weight, weight_sum,
             grad_scale=1.0):
    """Inputs: float32 arrays (`legal`: anything whose non-zero entries are legal).  `weight_sum` and `grad_scale` are
    arguments, as in the C ABI.  -> dict(terms [B,4] = kl, weight, bucket CE, WDL aux; g1, g2, g3 [B,36]; gv [B,101]; lp
    [B,220] log-probabilities; lo, hi), float64 numpy."""
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).astype(np.float64))
    B = int(np.asarray(lp1).shape[0])
    h1, h2, h3 = (f64(a).reshape(B, 36).requires_grad_(True) for a in (lp1, lp2, lpm))
    vl = f64(vlogits).reshape(B, BINS).requires_grad_(True)
    legal_t = torch.from_numpy(np.asarray(legal).reshape(B, TOTAL) != 0)
    tgt_p = f64(target).reshape(B, TOTAL)
    raw32 = torch.from_numpy(np.asarray(value, dtype=np.float32).reshape(B).copy())
    draw, mixed, lo, hi, frac = value_bins_fp32(raw32, soft, alpha, anti_draw)
    dw = float(np.float32(draw_weight))
    w = torch.where(draw, torch.tensor(dw, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    denom = float(np.float32(weight_sum)) + 1e-8
    gs = float(np.float32(grad_scale))

    # ---- forward, float64, under autograd ----
    kl, lp, p, live, lse_ok = _policy_forward(_combined(h1, h2, h3), legal_t, tgt_p)
    tgt_v = torch.zeros((B, BINS), dtype=torch.float64)
    tgt_v.scatter_add_(1, lo.view(-1, 1), (1.0 - frac).double().view(-1, 1))
    tgt_v.scatter_add_(1, hi.view(-1, 1), frac.double().view(-1, 1))
    vlog = torch.log_softmax(vl, dim=1)
    cev = -(tgt_v * vlog).sum(dim=1)
    probs = torch.softmax(vl, dim=1)
    pw, pl = probs[:, 50:].sum(dim=1), probs[:, :50].sum(dim=1)      # fp32 linspace(-1, 1, 101)[50] = 2.2e-8 > 1e-8: a WIN bin
    pd = torch.zeros_like(pw)                                        # ... so the draw class is empty
    s3 = (pw + pd + pl).clamp_min(1e-8)
    raw = raw32.double()
    tw, tl = raw.clamp(min=0.0), (-raw).clamp(min=0.0)
    td = (1.0 - tw - tl).clamp(min=0.0)
    aux = -(tw * (pw / s3).clamp_min(1e-8).log() + td * (pd / s3).clamp_min(1e-8).log() +
            tl * (pl / s3).clamp_min(1e-8).log())
    total = gs * ((kl * w).sum() / denom + cev.mean())
    g_auto = torch.autograd.grad(total, (h1, h2, h3, vl))

    # ---- the same gradients by hand ----
    with torch.no_grad():
        passes = live & (lp >= -50.0)                     # where(isfinite) and clamp(min=-50) both let the gradient through
        gl = torch.where(passes, -tgt_p * (gs * w / denom).view(-1, 1), torch.zeros_like(tgt_p)).numpy()
        dc = gl - p.numpy() * gl.sum(axis=1, keepdims=True)           # dL / d combined
        g1, g2 = dc[:, :36].copy(), np.zeros((B, 36))
        for m in range(144):
            if ON_BOARD[m]:                               # an off-board move is never live: its dc is 0 and has no target
                g1[:, MOVE_DEST[m]] += dc[:, 36 + m]
                g2[:, MOVE_FROM[m]] += dc[:, 36 + m]
        g3 = dc[:, 180:216].copy()
        gv = (probs - tgt_v).numpy() * (gs / B)
    for name, hand, auto in zip(("g1", "g2", "g3", "gv"), (g1, g2, g3, gv), g_auto):
        auto = auto.numpy()
        assert np.isfinite(hand).all() and np.isfinite(auto).all(), name
        err = np.abs(hand - auto).max(initial=0.0)
        assert err <= 1e-12 * max(1.0, gs), f"{name}: hand-written gradient differs from autograd by {err:.3e}"
    terms = torch.stack([kl, w, cev, aux], dim=1).detach().numpy()
    return dict(terms=terms, g1=g1, g2=g2, g3=g3, gv=gv, lp=lp.detach().numpy(), live=live.numpy(), lo=lo.numpy(),
                hi=hi.numpy(), mixed=mixed.numpy())


def run_oracle(c, setting, grad_scale=1.0):
    """oracle/loss_oracle.py (float32, CPU) on a case dict -> the same keys as ref_loss, float32."""
    from oracle.loss_oracle import policy_value_loss
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k]))
    leaves = [t(k).clone().requires_grad_(True) for k in ("lp1", "lp2", "lpm", "vlogits")]
    out = policy_value_loss(*leaves, t("mask") != 0, t("target"), t("value"), t("soft"), soft_label_alpha=setting[0],
                            anti_draw_penalty=setting[1], policy_draw_weight=setting[2])
    (out["loss"] * float(grad_scale)).backward()
    terms = torch.stack([out["kl"], out["weight"], out["ce_value"], out["wdl_aux"]], dim=1).detach().numpy()
    return dict(terms=terms, g1=leaves[0].grad.numpy(), g2=leaves[1].grad.numpy(), g3=leaves[2].grad.numpy(),
                gv=leaves[3].grad.numpy())


# The bounds of the kernel comparison (tests/test_gpu_train_kernels.py): (rtol, atol); the atol of the policy gradients
# is per unit of grad_scale, that of gv per unit of grad_scale / B.
BASE_TOL = dict(kl=(2e-5, 1e-5), ce=(2e-5, 1e-5), aux=(2e-5, 1e-5), g1=(1e-4, 1e-6), g2=(1e-4, 1e-6), g3=(1e-4, 1e-6),
                gv=(1e-4, 5e-5))
POLICY_QUANTITIES = ("kl", "g1", "g2", "g3")              # classed by the heads; ce, aux, gv by the value logits


def quantities(r):
    t = r["terms"]
    return dict(kl=t[:, 0], ce=t[:, 2], aux=t[:, 3], g1=r["g1"], g2=r["g2"], g3=r["g3"], gv=r["gv"])


def tolerance(name, B, grad_scale):
    rtol, atol = BASE_TOL[name]
    if name in ("g1", "g2", "g3"):
        atol *= grad_scale
    elif name == "gv":
        atol *= grad_scale / B
    return rtol, atol


def excess(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 means within the bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def wide_class_factors(c, classes_p, classes_v, want, setting, grad_scale):
    """For the wide classes the bound is not fixed in advance: the float32 oracle is measured against `want` (ref_loss) on
    the same rows, in units of the base bound; where that exceeds 1 the class's bound is 4 x the measured maximum (the
    kernel sums over a wave butterfly where the oracle sums in order, and uses the device expf / logf).  Never derived
    from the kernel's output.  -> {(quantity, class): factor >= 1}, {(quantity, class): measured}."""
    B = len(c["value"])
    got = quantities(run_oracle(c, setting, grad_scale))
    ref = quantities(want)
    factors, measured = {}, {}
    for name in BASE_TOL:
        cls = classes_p if name in POLICY_QUANTITIES else classes_v
        rtol, atol = tolerance(name, B, grad_scale)
        for k in np.unique(cls):
            rows = cls == k
            m = excess(got[name][rows], ref[name][rows], rtol, atol)
            measured[(name, str(k))] = m
            factors[(name, str(k))] = 1.0 if (k == "base" or m <= 1.0) else 4.0 * m
    return factors, measured


# =========================================================================================================================
# The 360-byte trajectory record: u64[4] {own | phase << 36, opp, own-marked, opp-marked}, u32[7] legal bits,
# f32[72] policy of the legal actions in ascending action order (zero-filled), f32 value, f32 soft, 4 zero bytes.
# -0.0 in a plane or in the policy off the legal set compares equal to zero: it is packed as a cleared bit / left out,
# raises no count and comes back as +0.0 -- the one exception to "unpack(pack(x)) reproduces every byte".
# =========================================================================================================================
def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ref_representable(rows):
    """bool[n]: planes 0/1, at most one phase plane and that one full, no policy off the legal set, <= 72 legal."""
    planes, legal, policy, _, _ = rows
    n = len(planes)
    ok = np.ones(n, bool)
    for s in range(n):
        pl = np.asarray(planes[s], np.float32).reshape(11, 36)
        good = bool(((pl == 0) | (pl == 1)).all())
        filled = [int((pl[p] != 0).sum()) for p in range(4, 11)]
        good &= all(f in (0, 36) for f in filled) and sum(f != 0 for f in filled) <= 1
        lg = np.asarray(legal[s]).reshape(TOTAL) != 0
        pol = np.asarray(policy[s], np.float32).reshape(TOTAL)
        good &= bool((pol[~lg] == 0).all())               # NaN off the mask is a defect, -0.0 is not
        good &= int(lg.sum()) <= POLICY_SLOTS
        ok[s] = good
    return ok


def ref_pack(rows):
    """(planes f32[n,11,6,6], legal u8[n,220], policy f32[n,220], value f32[n], soft f32[n]) -> (uint8[n,360], bad_count).
    The record of a row that is not representable is not specified (only counted)."""
    planes, legal, policy, value, soft = rows
    n = len(planes)
    out = np.zeros((n, RECORD_BYTES), np.uint8)
    for s in range(n):
        pl = np.asarray(planes[s], np.float32).reshape(11, 36)
        w = [0, 0, 0, 0]
        for p in range(4):
            for c in range(36):
                if pl[p, c] != 0:
                    w[p] |= 1 << c
        phase = 0
        for ph in range(1, 8):
            if (pl[3 + ph] != 0).any():
                phase = ph
        w[0] |= phase << 36
        m = [0] * 7
        pbits = _bits32(policy[s]).reshape(TOTAL)
        slots = []
        for a in range(TOTAL):
            if np.asarray(legal[s]).reshape(TOTAL)[a] != 0:
                m[a >> 5] |= 1 << (a & 31)
                if len(slots) < POLICY_SLOTS:
                    slots.append(pbits[a])
        rec = out[s]
        rec[0:32] = np.array(w, np.uint64).view(np.uint8)
        rec[32:60] = np.array(m, np.uint32).view(np.uint8)
        pv = np.zeros(POLICY_SLOTS, np.uint32)
        pv[:len(slots)] = slots
        rec[60:348] = pv.view(np.uint8)
        rec[348:352] = _bits32(value).reshape(-1)[s:s + 1].view(np.uint8)
        rec[352:356] = _bits32(soft).reshape(-1)[s:s + 1].view(np.uint8)
    return out, int((~ref_representable(rows)).sum())


def ref_unpack(records):
    """uint8[n,360] -> (planes f32[n,11,6,6], legal u8[n,220], policy f32[n,220], value f32[n], soft f32[n]).  Total: the
    phase is (w0 >> 36) & 7, bits the layout does not own are ignored, and a legal bit whose slot is >= 72 gets policy 0."""
    records = np.ascontiguousarray(records, dtype=np.uint8)
    n = records.shape[0]
    planes = np.zeros((n, 11, 36), np.float32)
    legal = np.zeros((n, TOTAL), np.uint8)
    policy = np.zeros((n, TOTAL), np.uint32)
    value, soft = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for s in range(n):
        rec = records[s]
        w = [int(x) for x in rec[0:32].copy().view(np.uint64)]
        m = [int(x) for x in rec[32:60].copy().view(np.uint32)]
        pv = rec[60:348].copy().view(np.uint32)
        for p in range(4):
            for c in range(36):
                planes[s, p, c] = (w[p] >> c) & 1
        phase = (w[0] >> 36) & 7
        if phase:
            planes[s, 3 + phase] = 1.0
        slot = 0
        for a in range(TOTAL):
            if (m[a >> 5] >> (a & 31)) & 1:
                legal[s, a] = 1
                policy[s, a] = pv[slot] if slot < POLICY_SLOTS else 0
                slot += 1
        value[s] = rec[348:352].copy().view(np.uint32)[0]
        soft[s] = rec[352:356].copy().view(np.uint32)[0]
    return (planes.reshape(n, 11, 6, 6), legal, policy.view(np.float32), value.view(np.float32), soft.view(np.float32))
