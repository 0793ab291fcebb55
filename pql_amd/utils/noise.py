"""Gaussian action noise with the reference's names (pql/utils/noise.py:19-41)."""
import math
from collections import namedtuple

import torch


def _draw(shape, dtype, device, std, generator=None):
    # torch.normal(zeros, std_tensor) consumes the generator as normal_(0,1) then scales (Appendix B of SURVEY.md)
    return torch.empty(shape, dtype=dtype, device=device).normal_(generator=generator) * std


_STD_CACHE = {}


def _fused(x, draw, std_rows, std_scalar, out_bounds, generator):
    """out = clamp(x + draw * sigma, lo, hi) in one launch (plus the draw itself) when x is a contiguous fp32 matrix on the GPU."""
    from pql_amd import _lib as L
    if draw is None:
        draw = torch.empty_like(x).normal_(generator=generator)   # torch.normal(zeros, std) = normal_(0,1) then the scale (Appendix B)
    else:
        draw = draw.to(x.dtype).contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        L.check(L.lib.pqlk_action_noise(L.ptr(x), L.ptr(draw), L.ptr(std_rows), float(std_scalar), x.shape[0], x.shape[1],
                                        float(out_bounds[0]), float(out_bounds[1]), L.ptr(out), L.stream(x.device)))
    return out


def _fusable(x, noise_bounds, out_bounds):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.numel() > 0 and noise_bounds is None
            and out_bounds is not None)


def add_normal_noise(x, std, noise_bounds=None, out_bounds=None, generator=None, draw=None):
    """`draw`: optional injected N(0,1) sample of x's shape (parity tests); otherwise drawn from `generator`."""
    if _fusable(x, noise_bounds, out_bounds) and not torch.is_tensor(std):
        return _fused(x, draw, None, std, out_bounds, generator)
    noise = _draw(x.shape, x.dtype, x.device, std, generator) if draw is None else draw.to(x.dtype) * std
    if noise_bounds is not None:
        noise = noise.clamp(noise_bounds[0], noise_bounds[1])
    out = x + noise
    return out if out_bounds is None else out.clamp(out_bounds[0], out_bounds[1])


def mixed_std_rows(rows, device, std_max, std_min, env_offset=0, total_envs=None):
    """(rows, 1) per-env sigma = linspace(std_min, std_max, N)[env_offset : env_offset + rows], N = total_envs or rows."""
    n = rows if total_envs is None else total_envs
    key = (float(std_min), float(std_max), int(n), int(env_offset), int(rows), str(device))
    std = _STD_CACHE.get(key)
    if std is None:   # built on the host like the reference (same fp32 values), uploaded ONCE: no per-step H2D sync
        std = torch.linspace(std_min, std_max, n)[env_offset: env_offset + rows].to(device).unsqueeze(-1)
        _STD_CACHE[key] = std
    return std


def add_mixed_normal_noise(x, std_max, std_min, noise_bounds=None, out_bounds=None, env_offset=0, total_envs=None,
                           generator=None, draw=None):
    """Per-env sigma = linspace(std_min, std_max, N)[env].  env_offset/total_envs let a data-parallel
    rank index the GLOBAL env axis."""
    std = mixed_std_rows(x.shape[0], x.device, std_max, std_min, env_offset, total_envs)
    if _fusable(x, noise_bounds, out_bounds):
        return _fused(x, draw, std, 0.0, out_bounds, generator)
    noise = (_draw(x.shape, x.dtype, x.device, 1.0, generator) if draw is None else draw.to(x.dtype)) * std
    if noise_bounds is not None:
        noise = noise.clamp(noise_bounds[0], noise_bounds[1])
    out = x + noise
    return out if out_bounds is None else out.clamp(out_bounds[0], out_bounds[1])


# ---- temporally correlated exploration noise (algo.noise.color) ---------------------------------------------------
COLORS = ("white", "ar1", "pink")
MAX_OCTAVES = 8   # PQLK_NOISE_MAX_OCTAVES
# algo.name of the agents whose exploration is a sample of their own stochastic policy (droq_algo is AgentSAC: name "SAC")
OWN_SAMPLERS = ("SAC", "TQC", "PPO")
ColorSpec = namedtuple("ColorSpec", "color groups octaves corr_min corr_max")   # groups = G, octaves = R of the law


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _whole(v):
    return _number(v) and int(v) == v


def noise_color(cfg):
    """`algo.noise.color` and its keys checked, before anything is allocated -> None (white, or a config without the keys: nothing
    of the coloured path exists) or the ColorSpec of the law (include/pqlk.h, pqlk_action_noise_colored).  Every key is read with
    its default and checked whatever the colour; a ValueError names the key."""
    algo = cfg.algo
    node = algo.get("noise") or {}
    color = node.get("color", "white")
    lo, hi = node.get("corr_min", 0.0), node.get("corr_max", 0.95)
    groups, octaves = node.get("corr_groups", 8), node.get("octaves", 6)
    if color not in COLORS:
        raise ValueError(f"algo.noise.color must be one of {' | '.join(COLORS)}, got {color!r}")
    for key, v in (("corr_min", lo), ("corr_max", hi)):
        if not _number(v) or not 0.0 <= float(v) < 1.0:
            raise ValueError(f"algo.noise.{key} must be a number in [0, 1) (the AR(1) coefficient of one step), got {v!r}")
    if float(lo) > float(hi):
        raise ValueError(f"algo.noise.corr_min must not be above algo.noise.corr_max, got corr_min={lo!r} > corr_max={hi!r}")
    if not _whole(groups) or int(groups) < 1:
        raise ValueError(f"algo.noise.corr_groups must be an integer >= 1 (correlation levels the envs cycle through), got {groups!r}")
    if not _whole(octaves) or not 1 <= int(octaves) <= MAX_OCTAVES:
        raise ValueError(f"algo.noise.octaves must be an integer in 1 ... {MAX_OCTAVES} (AR(1) processes summed per action), got {octaves!r}")
    if color == "white":
        return None
    name = str(algo.get("name") or "")
    if name in OWN_SAMPLERS:
        raise ValueError(f"algo.noise.color={color} cannot run with algo.name={name}: the agent explores by sampling its own policy and "
                         f"adds no action noise; algo.noise.color is taken by algo=pql_algo, algo=ddpg_algo and algo=crossq_algo")
    if color == "ar1":
        return ColorSpec(color, int(groups), 1, float(lo), float(hi))
    return ColorSpec(color, 1, int(octaves), 0.0, 0.0)


def color_tables(spec):
    """-> (rho (G, R) fp32, coef (G, R) fp32, w: a python float holding an fp32 value), on the host.
    ar1: rho = linspace(corr_min, corr_max, G) in fp32, like the sigma table; pink: rho = [0, 1 - 2^-1, ..., 1 - 2^-(R-1)], exact in
    fp32.  coef = fp32(sqrt(1 - rho^2)) evaluated in float64: every state has stationary variance 1; w = fp32(1 / sqrt(R))."""
    G, R = spec.groups, spec.octaves
    if spec.color == "ar1":
        rho = torch.linspace(spec.corr_min, spec.corr_max, G, dtype=torch.float32).reshape(G, 1)
    else:
        rho = torch.tensor([0.0] + [1.0 - 2.0 ** -k for k in range(1, R)], dtype=torch.float32).reshape(1, R)
    r64 = rho.to(torch.float64)
    coef = torch.sqrt(1.0 - r64 * r64).to(torch.float32)
    w = torch.tensor(1.0 / math.sqrt(R), dtype=torch.float64).to(torch.float32).item()
    return rho.contiguous(), coef.contiguous(), w


class ColoredNoise:
    """The state of the coloured exploration noise of `rows` envs x `cols` actions on one GPU, and its one launch per env step.
    The tables are built and uploaded once; `env_offset` is the first row's index on the GLOBAL env axis, so a data-parallel
    rank's rows take the correlation groups they have in the global run (the sigma rows are sliced by the caller the same way).
    state (rows, R, cols) and fresh (rows) uint8 are what a checkpoint keeps."""

    def __init__(self, spec, rows, cols, device, env_offset=0):
        from pql_amd import _lib as L
        device = torch.device(device)
        if device.type != "cuda":
            raise L.PqlkError(f"algo.noise.color={spec.color} runs on an MI355X device only (got {device}); pql_amd has no CPU path")
        self.spec, self.rows, self.cols, self.env_offset, self.device = spec, int(rows), int(cols), int(env_offset), device
        rho, coef, self.w = color_tables(spec)
        self.rho, self.coef = rho.to(device), coef.to(device)
        self.state = torch.zeros((self.rows, spec.octaves, self.cols), dtype=torch.float32, device=device)
        self.fresh = torch.ones(self.rows, dtype=torch.uint8, device=device)

    def reset(self):
        """Every row's process starts over at its next step."""
        self.fresh.fill_(1)

    def mark(self, done):
        """After an env step: the rows whose episode ended start over at the next step.  A device copy, no host sync."""
        self.fresh.copy_(done.reshape(-1))

    def step(self, act, std_rows=None, std_scalar=0.0, draw=None, generator=None, out_bounds=(-1.0, 1.0)):
        """out = clamp(act + n * sigma, lo, hi) with the states advanced by one step (in place) and `fresh` as it stands.
        `draw`: optional injected (rows, R * cols) N(0,1) sample; otherwise one `normal_` of that shape from `generator`."""
        from pql_amd import _lib as L
        R = self.spec.octaves
        if not (act.is_cuda and act.dtype == torch.float32 and tuple(act.shape) == (self.rows, self.cols)):
            raise L.PqlkError(f"coloured noise: the action must be a float32 ({self.rows}, {self.cols}) matrix on {self.device}, got "
                              f"{act.dtype} {tuple(act.shape)} on {act.device}")
        act = act.contiguous()
        if draw is None:
            draw = torch.empty((self.rows, R * self.cols), dtype=torch.float32, device=act.device).normal_(generator=generator)
        else:
            draw = draw.to(act.device, torch.float32).contiguous()
            if tuple(draw.shape) != (self.rows, R * self.cols):
                raise L.PqlkError(f"coloured noise: the injected draw must be ({self.rows}, {R * self.cols}), got {tuple(draw.shape)}")
        if std_rows is not None and (std_rows.numel() != self.rows or std_rows.dtype != torch.float32 or not std_rows.is_contiguous()):
            raise L.PqlkError(f"coloured noise: std_rows must hold {self.rows} contiguous float32 values")
        out = torch.empty_like(act)
        with torch.cuda.device(act.device):
            L.check(L.lib.pqlk_action_noise_colored(L.ptr(act), L.ptr(draw), L.ptr(std_rows), float(std_scalar), L.ptr(self.rho),
                                                    L.ptr(self.coef), self.spec.groups, R, self.env_offset, L.ptr(self.fresh),
                                                    L.ptr(self.state), self.rows, self.cols, self.w, float(out_bounds[0]),
                                                    float(out_bounds[1]), L.ptr(out), L.stream(act.device)))
        return out
