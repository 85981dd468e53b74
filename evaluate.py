#!/usr/bin/env python3
"""`python evaluate.py --arch A --dataset D --model_path run/checkpoints/final_checkpoint.pth` -- the reference's evaluate.py on the
MI355X path: test losses, hypervolume, rFID / PSNR / SSIM / LPIPS and gFID / IS / KID of a saved run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import movae_amd  # noqa: E402,F401
from movae_amd.saved_run import evaluate_main as main  # noqa: E402
from movae_amd.saved_run import evaluate_parser as build_parser  # noqa: E402,F401

if __name__ == "__main__":
    main()
