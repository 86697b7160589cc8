"""Child process of tests/test_gpu_replay_window.py::test_gather_trajectories_returns_the_records...: in a world-size-1
`nccl` group (as tests/nccl_world1.py sets one up) `gather_trajectories(..., as_records=True)` must return exactly
`pack_batch(batch)`, forced through the protocol or not.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", sys.argv[1] if len(sys.argv) > 1 else "29613")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    out = {"world": dist.get_world_size()}
    try:
        from liuzhou_amd.distributed import gather_trajectories
        from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
        from liuzhou_amd.self_play_gpu_runner import self_play_v1_gpu
        from liuzhou_amd.trajectory_codec import RECORD_BYTES, pack_batch
        torch.manual_seed(7)
        model = ChessNet(**MODEL_CONFIGS["tiny"]).eval().to(dev)
        mine, _ = self_play_v1_gpu(model, num_games=5, mcts_simulations=8, temperature_init=1.0, temperature_final=0.1,
                                   temperature_threshold=10, exploration_weight=1.0, device="cuda:0",
                                   add_dirichlet_noise=True, sample_moves=True, concurrent_games=5, max_game_plies=12,
                                   autocast_dtype="float32")
        want = pack_batch(mine)
        got = gather_trajectories(mine, dst=0, force=True, as_records=True)       # the protocol, records kept
        out["rows"] = int(mine.num_samples)
        out["records_shape_ok"] = got.dtype == torch.uint8 and tuple(got.shape) == (mine.num_samples, RECORD_BYTES) and got.is_cuda
        out["forced_equals_pack_batch"] = bool(torch.equal(got, want))
        out["unforced_equals_pack_batch"] = bool(torch.equal(gather_trajectories(mine, dst=0, as_records=True), want))
        out["default_returns_the_batch"] = gather_trajectories(mine, dst=0) is mine
    finally:
        dist.destroy_process_group()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
