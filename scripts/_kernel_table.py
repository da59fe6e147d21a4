"""What the kernel tables of the robust rules share (robust_kernel_table.py, q8_robust_kernel_table.py,
cclip_kernel_table.py): the buffers, the command line, the interleaved timing and the way a table is written."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BUFFERS = (("gpt2-small 124M", 124_439_808), ("268M", 268_435_456))


def parse_args(script, doc, out, reps, argv=None):
    """--out, --reps and --peers of the table script `script` (its __file__) with the module docstring `doc`; ends
    the run without a GPU."""
    ap = argparse.ArgumentParser(description=doc.splitlines()[0])
    ap.add_argument("--out", default=out)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--peers", type=int, nargs="+", default=[4, 8], help="peer counts P of the rows (1..16)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit(f"{Path(script).stem}: no GPU, nothing measured")
    return a


def time_interleaved(fn, reps, warmup=5):
    """Median / min ms per launch of each fn in `fn` (a dict), launches interleaved."""
    for _ in range(warmup):
        for f in fn.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fn}
    for _ in range(reps):
        for k, f in fn.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def write_table(lines, out):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(text)
