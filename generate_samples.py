#!/usr/bin/env python3
"""`python generate_samples.py --checkpoint run/checkpoints/final_checkpoint.pth [--prior_checkpoint run] --save_grid` -- the
reference's generate_samples_pixelcnn_vqvae*.py for every architecture: images drawn from a saved run, written as one grid or one
PNG per image."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import movae_amd  # noqa: E402,F401
from movae_amd.saved_run import generate_samples_main as main  # noqa: E402
from movae_amd.saved_run import generate_samples_parser as build_parser  # noqa: E402,F401

if __name__ == "__main__":
    main()
