"""recalgorithm_amd.algorithm.DIEN — part of the MI355X-native hot-path mirror."""
