#!/usr/bin/env python3
"""`python train_prior.py --checkpoint run/checkpoints/final_checkpoint.pth` -- the reference's train_prior_vqvae.py and
train_prior_vqvae2.py as one tool: a PixelCNN prior trained on the codes of a saved VQ-VAE or VQ-VAE-2."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import movae_amd  # noqa: E402,F401
from movae_amd.saved_run import train_prior_main as main  # noqa: E402
from movae_amd.saved_run import train_prior_parser as build_parser  # noqa: E402,F401

if __name__ == "__main__":
    main()
