"""prancSTR: the mosaic allele fit of every call (host layer of the trk_mosaic_fit device pass)."""
from .prancSTR import (ComputePvalue, ConfineRange, ExtractAB, ExtractReadVector, MaximizeMosaicLikelihoodBoth, SF,
                       StutterProb, mosaic_fit_records, mosaic_fit_vcf, read_counts, stutter_triple)
