"""Gradient-compression kernels alone, for counter runs: top-k 1% with error feedback, PowerSGD
rank 4 (lazy error feedback) and q8 (8-bit blocks with error feedback) over a flat bf16 gradient of
16 Linear(4096, 4096) layers (268M parameters, the Llama-3-8B projection shape), 4 rounds each,
single peer. q8 runs its three stages in the layout of Q8_PEERS peers: the encoded wire holds one
record per peer, which the reduce stage reads as if they were the peers' copies of one shard.

    python scripts/compress_only.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributedvolunteercomputing_amd.parallel.compression import PowerSGDCompressor, TopKCompressor  # noqa: E402
from distributedvolunteercomputing_amd.parallel.compression import Quant8Compressor  # noqa: E402
from distributedvolunteercomputing_amd.parallel.flat_params import FlatParams  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)
m = torch.nn.Sequential(*[torch.nn.Linear(4096, 4096, bias=False) for _ in range(16)]).to(dev, torch.bfloat16)
flat = FlatParams(m)
g = (torch.randn(flat.numel, device=dev) * 0.01).to(torch.bfloat16)
topk = TopKCompressor(flat.numel, 0.01, dev)
psgd = PowerSGDCompressor(flat, rank=4, device=dev)
Q8_PEERS = 8
q8 = Quant8Compressor(flat.numel, dev)
for _ in range(4):
    topk.allreduce_mean(g, None)
    psgd.allreduce_mean(g, None)
    wire = q8.encode(g, Q8_PEERS)
    q8.reduce(wire, Q8_PEERS)
    q8.decode(wire, Q8_PEERS)
torch.cuda.synchronize()
L, m, rec = q8.layout(Q8_PEERS)
print(f"[compress_only] n={flat.numel} topk ratio={1 / topk.ratio:.1f} psgd ratio={psgd.compression_ratio:.1f} "
      f"q8 peers={Q8_PEERS} L={L} shard={m} record_bytes={rec} "
      f"wire_bytes_per_element={2 * (Q8_PEERS - 1) * rec / flat.numel:.4f} "
      f"(bf16 direct: {2 * 2 * (Q8_PEERS - 1) / Q8_PEERS:.4f})")
