"""AutoInt (Song et al., CIKM 2019): the upstream zoo lists it as to do and ships no file; the surface follows algorithm/AFM."""
