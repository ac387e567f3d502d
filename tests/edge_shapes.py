"""Capacity edges of the fused kernel families, derived from the admission rules themselves (tensorbnn_amd/jit.py: `families`, `mid_usage`,
`tall_usage`, `wide_usage`, `narrow_usage`): no random draws.  Each case starts from a small shape its family takes, walks one dimension (fan-in, a
hidden width, the output count, or the depth: one more copy of the last hidden layer) while the family still admits the shape, and records the last
admitted shape (`dims`) and its first refused neighbour (`refused`).  A depth walk ends at the C ABI's 16 dense layers at the latest (limit "abi").  `limit` names the rule that refuses the neighbour; tests/test_host_logic.py recomputes the estimates and checks that it is that rule
alone, tests/test_gpu_capacity.py runs both shapes against the fp64 oracle.  __graft_entry__.build() prebuilds their run-time instantiations
(`jit_jobs`).

A case: dict(name, family, dims, refused, limit, lik) -- `family` is what jit.families calls the kernel ("fast3", "fast", "mid", "tall", "wide");
`refused` is None where the pair is two admitted shapes (the VALU / MFMA last layer of mid; the fan-in at which `wide_fits` starts to apply)."""
import os

ACT_TANH = 2
LIK_GAUSSIAN, LIK_BERNOULLI = 0, 2
PRIOR_CAUCHY = 0

# TBNN_JIT_SKIP that makes `family` take an admitted shape
SKIP = {"fast3": "mid,tall,wide", "fast": "fast3,mid,tall,wide", "mid": "fast3,fast,tall,wide", "tall": "fast3,fast,mid,wide",
        "wide": "fast3,fast,mid,tall"}
NARROW_MAX_FANIN, NARROW_MAX_WIDTH = 16, 64

MAX_LAYERS = 16                   # include/tbnn.h: TBNN_MAX_LAYERS (tbnn_create refuses deeper networks)
DEPTH = "depth"

# (name, family, base dims, index walked, step, limit): the walk moves dims[index] by step (+1 or -1) from the base while `family` is in
# families(dims); index DEPTH inserts a copy of the last hidden layer instead (step +1)
WALKS = [
    # narrow: every dW tile in one wave's registers
    ("narrow-fanin", "fast3", [8, 32, 32, 1], 0, +1, "fanin"),
    ("narrow-width", "fast3", [8, 32, 32, 1], 1, +1, "width"),
    ("narrow-tiles", "fast3", [16, 64, 64, 16, 1], 3, +1, "tiles"),
    ("narrow-onehidden", "fast3", [8, 64, 2], 1, +1, "onehidden"),
    ("narrow-onehidden-many", "fast", [9, 64, 16], 1, +1, "onehidden"),
    # mid: AccVGPR tiles, LDS, outputs
    ("mid-fanin", "mid", [20, 32, 32, 1], 0, +1, "fanin"),
    ("mid-tiles", "mid", [32, 64, 96, 2], 1, +1, "tiles"),
    ("mid-lds", "mid", [128, 16, 16, 1], 1, +1, "lds"),
    ("mid-outputs", "mid", [20, 48, 48, 3], 3, +1, "outputs"),
    # tall: fan-in split over four waves, W_0 / dW_0 in registers
    ("tall-fanin-onehidden", "tall", [40, 32, 1], 0, -1, "fanin"),
    ("tall-fanin", "tall", [48, 32, 32, 1], 0, -1, "fanin"),
    ("tall-hidden", "tall", [100, 48, 32, 1], 1, +1, "hidden"),
    # (one hidden layer: `tall_limits` allows 128 units, but from 113 the exchange buffer and dW_0 staging alone take 160 KB -- the LDS bound
    # is what refuses, at every fan-in)
    ("tall-hidden-onehidden", "tall", [100, 64, 1], 1, +1, "lds"),
    ("tall-vgpr", "tall", [300, 64, 16, 1], 0, +1, "vgpr"),
    # (the VGPR + AGPR bound of 500 never binds alone any more: where `regs` <= 340 holds, so does it, or the VGPR bound binds first)
    ("tall-regs", "tall", [41, 64, 56, 2], 0, +1, "regs"),
    ("tall-regs-width", "tall", [36, 16, 56, 16, 2], 3, +1, "regs"),
    ("tall-lds", "tall", [33, 40, 3], 1, +1, "lds"),
    # wide: W_0 in LDS next to the weight ring
    ("wide-fanin", "wide", [40, 64, 64, 1], 0, +1, "fanin"),
    ("wide-hidden", "wide", [10, 200, 200, 1], 2, +1, "hidden"),
    ("wide-tiles0", "wide", [128, 64, 64, 1], 1, +1, "tiles0"),
    ("wide-lds", "wide", [40, 80, 256, 1], 0, +1, "lds"),
    ("wide-regs", "wide", [8, 256, 240, 1], 0, +1, "regs"),
    ("wide-outputs", "wide", [10, 200, 120, 3], 3, +1, "outputs"),
    # depth: every layer adds weight and activation images to the LDS plans of narrow, mid and tall; the wide family streams its middle
    # layers through a ring of weight slots and reaches the ABI's 16 layers
    ("narrow-depth", "fast3", [4, 16, 16, 1], DEPTH, +1, "lds"),
    ("narrow-depth-fast", "fast", [4, 16, 16, 1], DEPTH, +1, "lds"),
    ("mid-depth", "mid", [4, 16, 16, 2], DEPTH, +1, "abi"),
    ("mid-depth-outputs", "mid", [4, 24, 24, 10], DEPTH, +1, "lds"),
    ("tall-depth", "tall", [300, 16, 16, 2], DEPTH, +1, "lds"),
    ("wide-depth", "wide", [10, 64, 64, 1], DEPTH, +1, "abi"),
]
# pairs of admitted shapes on one family (refused None)
PAIRS = [
    # the same widths with a VALU (2 outputs) and an MFMA (3 outputs) last layer, 8 KB under the LDS bound (with 3 .. 16 outputs the LDS
    # bound binds before the 63rd tile: mid-tiles' 63-tile shape with 3 outputs is refused)
    ("mid-valu-mfma", "mid", [20, 100, 48, 2], [20, 100, 48, 3], "last-layer"),
    # fan-in 32 (only the register estimate) and 33 (`wide_fits`' LDS and dW_0 estimates apply too)
    ("wide-fanin32", "wide", [32, 192, 192, 1], [33, 192, 192, 1], "wide_fits"),
]
# edges also run with a Bernoulli likelihood (sigmoid last layer, outputs kept off saturation): one per family
BERNOULLI = ("narrow-tiles", "narrow-onehidden-many", "mid-tiles", "tall-regs", "wide-regs")
WALK_CAP = 4096
# shapes whose fused build spills (tests/golden/jit_build_outcomes.json has the measurements): the estimates must refuse them -- earlier edges of
# this list's walks, and the fuzz draws of fuzz_shapes.UNBUILDABLE that still spill
MUST_REFUSE = {
    ("tall", (575, 48, 64, 64, 1)): "k_fwd_bwd_tall spills 928 bytes per lane (the old VGPR + AGPR edge)",
    ("tall", (511, 32, 64, 64, 3)): "k_fwd_bwd_tall spills 208 bytes per lane (the old LDS edge)",
    ("tall", (362, 49, 64, 1)): "k_fwd_bwd_tall spills 48 bytes per lane",
    ("tall", (525, 39, 64, 22, 2)): "k_fwd_bwd_tall spills 432 bytes per lane",
    ("wide", (32, 256, 256, 1)): "k_chain_wide spills 196 bytes per lane",
    ("wide", (33, 256, 256, 1)): "k_chain_wide spills 260 bytes per lane",
}
# fuzz_shapes.UNBUILDABLE draws the estimates admit and the build now takes (tanh hidden layers): tests/test_gpu_capacity.py runs them
UNBUILDABLE_ADMITTED = [("wide", [19, 148, 191, 1]), ("wide", [26, 234, 229, 115, 1]), ("wide", [26, 234, 229, 115, 2])]


def _families(dims):
    from tensorbnn_amd import jit
    return jit.families(dims)


def admits(family, dims):
    return family in _families(dims)


def _step(dims, index, step):
    d = list(dims)
    if index == DEPTH:
        return d[:-1] + [d[-2]] + d[-1:]
    d[index] += step
    return d


def walk(family, base, index, step):
    """(last admitted shape, first refused neighbour) along one dimension"""
    assert admits(family, base), (family, base)
    d = list(base)
    for _ in range(WALK_CAP):
        nxt = _step(d, index, step)
        if min(nxt) < 1 or not admits(family, nxt):        # (a network deeper than MAX_LAYERS: no family, `abi`)
            return d, nxt
        d = nxt
    raise AssertionError(f"{family}: no limit within {WALK_CAP} steps of {base}")


def cases():
    out = []
    for name, fam, base, index, step, limit in WALKS:
        dims, refused = walk(fam, base, index, step)
        out.append(dict(name=name, family=fam, dims=dims, refused=refused, limit=limit, lik=LIK_GAUSSIAN))
        if name in BERNOULLI:
            out.append(dict(name=name + "-bern", family=fam, dims=dims, refused=None, limit=limit, lik=LIK_BERNOULLI))
    for name, fam, a, b, limit in PAIRS:
        out.append(dict(name=name, family=fam, dims=a, refused=None, limit=limit, lik=LIK_GAUSSIAN))
        out.append(dict(name=name + "-b", family=fam, dims=b, refused=None, limit=limit, lik=LIK_GAUSSIAN))
    for k, (fam, dims) in enumerate(UNBUILDABLE_ADMITTED):
        out.append(dict(name=f"unbuildable-draw{k}", family=fam, dims=dims, refused=None, limit="none", lik=LIK_GAUSSIAN))
    return out


def usage(family, dims) -> dict:
    """{limit: (value, bound)} of every admission rule of `family` (the rules of jit.families restated; the estimates from jit's *_usage):
    `family` admits `dims` exactly when no value exceeds its bound"""
    from tensorbnn_amd import jit
    nl, out = len(dims) - 1, dims[-1]
    if family in ("fast3", "fast"):
        tiles = sum(jit._cdiv(dims[l + 1], 16) * jit._cdiv(dims[l] + 1, 16) for l in range(nl))
        u = {"fanin": (dims[0], NARROW_MAX_FANIN), "tiles": (tiles, jit.NARROW_TILES), "abi": (nl, MAX_LAYERS)}
        if nl == 2:
            u["onehidden"] = (max(dims), 256 if out <= 2 else 160)
        else:
            u["width"] = (max(dims), NARROW_MAX_WIDTH)
        if family == "fast3":
            u["outputs"] = (out, 2)
        # (the LDS plan is only evaluated for shapes the narrow rules above admit, as jit.families does)
        if all(v <= b for v, b in u.values()):
            u["lds"] = (jit.narrow_usage(dims)[family], jit.NARROW_LDS)
        return u
    u = {"depth": (0 if nl >= (2 if family == "tall" else 3) else 1, 0), "outputs": (out, 16), "abi": (nl, MAX_LAYERS)}
    if family == "mid":
        u["fanin"] = (dims[0], jit.MID_MAX_FANIN)
        est, lim = jit.mid_usage(dims), jit.MID_LIMITS
    elif family == "tall":
        u["fanin"] = (-dims[0], -(17 if nl == 2 else 33))                # (a LOWER bound: fan-in 17 / 33 and up)
        est, lim = jit.tall_usage(dims), jit.tall_limits(dims)
    else:
        u["fanin"] = (dims[0], 128)
        u["hidden"] = (max(dims[1:-1]), 256)
        est, lim = jit.wide_usage(dims), {k: v for k, v in jit.WIDE_LIMITS.items() if k == "regs" or dims[0] > 32}
    u.update({k: (est[k], lim[k]) for k in lim})
    return u


def over(family, dims) -> set:
    """the rules of `family` that `dims` breaks"""
    return {k for k, (v, b) in usage(family, dims).items() if v > b}


def landing(dims):
    """the family a refused neighbour runs on with no TBNN_JIT_SKIP: the first of families(), or "layered"; "abi" where tbnn_create refuses
    the network"""
    if len(dims) - 1 > MAX_LAYERS:
        return "abi"
    f = [x for x in _families(dims)]
    return f[0] if f else "layered"


def layers_of(dims, lik=LIK_GAUSSIAN, act=ACT_TANH):
    last = 3 if lik == LIK_BERNOULLI else 0          # sigmoid / none
    return [[dims[i], dims[i + 1], act if i < len(dims) - 2 else last, PRIOR_CAUCHY] for i in range(len(dims) - 1)]


def jit_jobs():
    """the run-time instantiations tests/test_gpu_capacity.py asks for, as jit.prebuild takes them"""
    jobs = []
    for c in cases():
        jobs.append({"layers": layers_of(c["dims"], c["lik"]), "likelihood": c["lik"], "skip": SKIP[c["family"]], "flags": ""})
        if c["refused"] is not None and landing(c["refused"]) not in ("layered", "abi"):
            jobs.append({"layers": layers_of(c["refused"], c["lik"]), "likelihood": c["lik"], "skip": "", "flags": ""})
    return jobs


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tensorbnn_amd import jit
    for c in cases():
        r = c["refused"]
        print(f"{c['name']:24s} {c['family']:5s} {str(c['dims']):26s} -> {str(r):26s} {c['limit']:10s} "
              f"lands {landing(r) if r else '-':8s} mid {jit.mid_usage(c['dims'])} tall {jit.tall_usage(c['dims'])} wide {jit.wide_usage(c['dims'])}")
    print(len(jit_jobs()), "instantiations")
