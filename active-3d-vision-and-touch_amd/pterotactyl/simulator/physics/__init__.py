"""The grasp of the reference's ``simulator/physics``: hand placement restated, finger closing by a kinematic rule (``grasping.py``)."""
