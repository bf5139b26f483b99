"""One rank of a two-device RCCL run of the momentum terms (started by tests/test_gpu_momentum_terms.py, one process per GPU): two RK3
steps on this rank's tile, then the rank-local csi_momentum_terms_compute and the collective csi_momentum_budget_compute; the fields, the
five powers and the tile's offsets go to <out>.rank<r>.npz."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    rank, world, port, Rx, Ry, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
    kw = json.loads(sys.argv[7])
    kw["topo"] = tuple(kw["topo"])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import numpy as np
    import torch
    import torch.distributed as dist
    import cases
    import momentum_terms_ref as ref
    from test_gpu_momentum_terms import STEP_KW, _run
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{rank}"))
    try:
        c = cases.make_case(substeps=8, random_uv=0.02, **kw)
        m = cases.csi_model(c, device=f"cuda:{rank}", tile=(Rx, Ry, rank), **STEP_KW)
        fields, b = _run(m, c)
        np.savez(f"{out}.rank{rank}.npz", budget=np.array([b[k] for k in ref.TERMS]), offsets=np.array([m.grid.i_off, m.grid.j_off]), **fields)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
