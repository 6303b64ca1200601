"""Host-side mirror of the reference's util package, restricted to the mesh output of util/visualize.py."""
