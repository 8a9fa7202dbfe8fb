"""Mirror of the reference's algorithm/WideAndDeep."""
