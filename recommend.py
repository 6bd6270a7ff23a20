#!/usr/bin/env python3
"""``python recommend.py ...`` -- top-K recommendations for a CSV's users from saved weights; see amid_amd/recommend.py."""
from amid_amd.recommend import main

if __name__ == "__main__":
    main()
