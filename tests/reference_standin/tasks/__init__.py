"""Stand-in package (see ../README.md)."""
