"""Empty stand-in: the reference imports it at data/datasets/scannet_old.py:9 and never calls it in __getitem__."""
