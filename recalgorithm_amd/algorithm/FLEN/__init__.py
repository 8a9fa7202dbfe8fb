"""FLEN: field-wise bi-interaction with Dicefactor (Chen et al., arXiv 1911.04690); flen.py is the entry point."""
