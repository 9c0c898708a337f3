#!/usr/bin/env python3
"""Entry point with the reference's name: IJB-B / IJB-C template verification, TAR@FAR, on MI355X
(lafs_cvpr2024_amd/ijb_evaluation.py)."""
from lafs_cvpr2024_amd.ijb_evaluation import main

if __name__ == "__main__":
    main()
