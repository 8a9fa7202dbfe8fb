"""Mirror of /root/reference algorithm/MMOE."""
