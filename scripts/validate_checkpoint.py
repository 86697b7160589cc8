#!/usr/bin/env python3
"""Validation metrics of a checkpoint on the rows of a self-play stage (`liuzhou_amd/validation.py`), for the file-based
pipeline: the checkpoint as `scripts/train_stage.py --load_checkpoint` reads it, the rows through the reader
`train_stage.py` uses for `--self_play_input` (a manifest's chunk files or a single payload).  Meaningful when the
checkpoint was NOT trained on these rows: validate generation i with the checkpoint of generation i-1, before
`train_stage.py` consumes it.

    python scripts/validate_checkpoint.py --load_checkpoint ckpt/model_iter_007.pt --self_play_input sp/iter_008.json

One JSON line: the result dict of `validate_network` plus the inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--load_checkpoint", default=None, help="model_state_dict checkpoint; without it --model at its seeded init")
    ap.add_argument("--model", default="b10c128", choices=["b6c64", "b10c128"])
    ap.add_argument("--model_init_seed", type=int, default=int(os.environ.get("V1_MODEL_INIT_SEED", "20260314")))
    ap.add_argument("--self_play_input", required=True)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--batch_size", type=int, default=4096)
    ap.add_argument("--evaluator", default="module", choices=["module", "fused"])
    ap.add_argument("--use_amp", type=int, default=1, choices=[0, 1])
    ap.add_argument("--soft_label_alpha", type=float, default=0.0)
    ap.add_argument("--max_rows", type=int, default=0, help="> 0: a seeded subset without replacement")
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = parse(argv)
    import torch
    from liuzhou_amd import self_play_stage as S
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.self_play_worker import _infer_model
    from liuzhou_amd.validation import validate_network
    if args.load_checkpoint:
        ck = torch.load(args.load_checkpoint, map_location="cpu", weights_only=False)
        state = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
        model = _infer_model(state)
        model.load_state_dict(state, strict=True)
    else:
        model = ChessNet(**MODEL_CONFIGS[args.model])
        if int(args.model_init_seed) > 0:
            stable_resnet_init(model, int(args.model_init_seed))
    model.to(args.device).eval()
    samples = S.concat_batches([S.load_self_play_payload(args.self_play_input)[0]])
    out = validate_network(model, samples, batch_size=args.batch_size, evaluator=args.evaluator, use_amp=bool(args.use_amp),
                           soft_label_alpha=args.soft_label_alpha, device=args.device, max_rows=args.max_rows, seed=args.seed)
    out.update(checkpoint=args.load_checkpoint, self_play_input=args.self_play_input, rows_in_input=int(samples.num_samples))
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
