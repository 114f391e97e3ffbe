"""Empty stand-in: the reference imports it at data/datasets/scannet_old.py:10 and never calls it in __getitem__."""
