"""ESMM (no upstream directory: built from the paper, see esmm.py)."""
