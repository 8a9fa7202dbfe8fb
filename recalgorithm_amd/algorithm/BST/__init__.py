"""recalgorithm_amd.algorithm.BST — part of the MI355X-native hot-path mirror."""
