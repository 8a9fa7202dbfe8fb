"""DCN-V2 (Wang et al., WWW 2021): the successor of algorithm/DCN; the upstream zoo ships no file, the surface follows DCN's."""
