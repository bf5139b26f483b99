"""One rank of a two-device RCCL run of the regional reduction (started by tests/test_gpu_regions.py, one process per GPU): one momentum
step on this rank's tile, then the collective csi_regions_compute on this rank's piece of the map; the record goes to
<out>.rank<r>.json (doubles as hex)."""
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
    threshold = float(sys.argv[8])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch
    import torch.distributed as dist
    import cases
    import climaseaice_jl_amd as csi
    from test_gpu_regions import as_plain, tile_ids
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{rank}"))
    try:
        c = cases.make_case(**kw)
        m = cases.csi_model(c, mode="fast", device=f"cuda:{rank}", tile=(Rx, Ry, rank))
        csi.time_step_momentum(m, c["dt"])
        ids, _ = tile_ids(c["Nx"], c["Ny"])
        r = csi.Regions(m.grid, ids, names=("a", "b", "c", "d"))
        with open(f"{out}.rank{rank}.json", "w") as f:
            json.dump(as_plain(m.regional_diagnostics(r, extent_threshold=threshold)), f)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
