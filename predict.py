#!/usr/bin/env python3
"""Predict masks with a trained checkpoint: one PNG per input image at the source resolution and / or the
run-length CSV (``img,rle_mask``) of the Carvana scoring.

    python3 predict.py -c singleGPU --input data/test_hq --output masks/ --rle submission.csv
    python3 predict.py -l checkpoints/DDP.pth --input a.jpg b.jpg --rle out.csv --img-size 512 -b 32
    python3 predict.py -c singleGPU --input data/test_hq --rle submission.csv --clean largest+fill

On a GPU the up-scale to the source size, the threshold and the run-length encoding run as HIP kernels
(csrc/predict_post.hip), bit-equal to the host path (PIL + numpy) that ``--host-post`` selects and a CPU-only
machine uses (see distributedpytorch_amd/predict.py).
"""
import warnings

warnings.filterwarnings("ignore")

from distributedpytorch_amd.predict import main  # noqa: E402

if __name__ == "__main__":
    main()
