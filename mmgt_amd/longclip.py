"""The long-clip options of the sampler, pure integers and doubles on the host: windows that do not wrap (`open_ended`), position weights
of the overlap average (`fuse_weights`), the steps that run both CFG rows (`check_guidance_interval`, `step_is_guided`), and the scripts' flags.

`get_context_scheduler` is the pipeline's window-list lookup: "open" is `open_ended`, every other name is context.get_context_scheduler's.  These
live beside mmgt_amd/context.py, not in it: that file mirrors the reference's schedule, and its text is part of the key of every committed oracle
result (tests/oracle_cache.py), none of which this module can change.
"""
from typing import Callable, Iterator, List

from . import context


def open_ended(step: int, num_steps, num_frames: int, context_size: int, context_stride: int = 1,
               context_overlap: int = 4) -> Iterator[List[int]]:
    """Open-ended windows: starts 0, s, 2 s, ... with s = context_size - context_overlap, and a last window that ends on the clip's last
    frame.  Never wrapped, all of context_size frames, every frame covered.  `step` and `num_steps` are taken for `uniform`'s signature only."""
    if context_stride != 1:
        raise ValueError(f"context_stride={context_stride} is not combined with context_schedule='open' (its windows hold consecutive frames): "
                         "use context_stride=1")
    if not 0 <= context_overlap < context_size:
        raise ValueError(f"context_overlap={context_overlap} must lie in 0 .. context_size - 1 = {context_size - 1} (the windows would not advance)")
    if num_frames <= context_size:
        yield list(range(num_frames))
        return
    s = context_size - context_overlap
    for j in list(range(0, num_frames - context_size, s)) + [num_frames - context_size]:
        yield list(range(j, j + context_size))


CONTEXT_FUSES = ("flat", "pyramid", "ramp")


def fuse_weights(name: str, n: int, context_overlap: int = 4) -> List[float]:
    """The per-position weights of a window of n frames in the overlap average, as Python doubles; the caller rounds them once to fp32.
    flat: 1;  pyramid: min(k + 1, n - k);  ramp: min(1, (k + 1) / (o + 1), (n - k) / (o + 1)) with o = context_overlap."""
    if name == "flat":
        return [1.0] * n
    if name == "pyramid":
        return [float(min(k + 1, n - k)) for k in range(n)]
    if name == "ramp":
        if context_overlap < 0:
            raise ValueError(f"context_fuse='ramp' with context_overlap={context_overlap}: the overlap must not be negative")
        o = context_overlap + 1
        return [min(1.0, (k + 1) / o, (n - k) / o) for k in range(n)]
    raise ValueError(f"Unknown context_fuse {name!r} (one of {', '.join(CONTEXT_FUSES)})")


def check_guidance_interval(interval):
    """None, or (lo, hi) with 0 <= lo < hi <= 1 -> None when every step is guided (None or (0, 1)), else (lo, hi) as floats."""
    if interval is None:
        return None
    try:
        lo, hi = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_interval must be None or a pair (lo, hi), got {interval!r}") from None
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError(f"guidance_interval must satisfy 0 <= lo < hi <= 1, got guidance_interval=({lo}, {hi})")
    return None if (lo, hi) == (0.0, 1.0) else (lo, hi)


def step_is_guided(t: int, interval, num_train_timesteps: int = 1000) -> bool:
    """Guidance in a limited interval (Kynkaanniemi et al., arXiv 2404.07724): with u = (t + 1) / num_train_timesteps the step at timestep t runs
    both CFG rows iff lo < u <= hi; every other step runs the conditional row alone."""
    if interval is None:
        return True
    lo, hi = interval
    return lo < (int(t) + 1) / num_train_timesteps <= hi


def get_context_scheduler(name: str) -> Callable:
    """ "open" -> `open_ended`; "uniform" (and the refusal of anything else) as context.get_context_scheduler"""
    if name == "open":
        return open_ended
    return context.get_context_scheduler(name)


def add_longclip_arguments(parser) -> None:
    """--context_schedule, --context_fuse and --guidance_interval of the scripts."""
    parser.add_argument("--context_schedule", default="uniform", choices=["uniform", "open"],
                        help="the window list: the reference's closed loop (the last window wraps to the clip's start), or open-ended windows")
    parser.add_argument("--context_fuse", default="flat", choices=list(CONTEXT_FUSES),
                        help="weights of a window's positions in the overlap average: flat (the reference), pyramid, or ramp (a linear cross-fade)")
    parser.add_argument("--guidance_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                        help="guide only the steps with LO < (t + 1) / 1000 <= HI; the other steps run the conditional row alone (2404.07724)")


def longclip_kwargs(args) -> dict:
    """The pipeline keywords of `add_longclip_arguments`; a default is not handed over."""
    kw = {}
    if args.context_schedule != "uniform":
        kw["context_schedule"] = args.context_schedule
    if args.context_fuse != "flat":
        kw["context_fuse"] = args.context_fuse
    if args.guidance_interval is not None:
        kw["guidance_interval"] = tuple(args.guidance_interval)
    return kw
