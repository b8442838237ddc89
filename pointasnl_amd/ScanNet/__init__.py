"""The ScanNet side of the reference (ScanNet/): the grid test and validation loops on the device (scene_tester)."""
