"""Mirror of the reference's algorithm/PLE."""
