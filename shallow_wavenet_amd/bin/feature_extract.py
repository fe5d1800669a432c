#!/usr/bin/env python3
"""stage 1 of run.sh for the features computed on the device (log-mel, mel-cepstrum of the short-time spectrum or of the F0-adaptive
envelope, F0 and voicing, band aperiodicity) - the reference's stage-1 flag names where they apply; see
shallow_wavenet_amd/feature_extract_driver.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from shallow_wavenet_amd.feature_extract_driver import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
