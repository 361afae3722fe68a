"""Mirror of the reference's ``pterotactyl/simulator``: the hand description (``hand.py``) and the grasp (``physics/grasping.py``).
**The finger closing is a kinematic rule, not Bullet's dynamics**: see ``physics/grasping.py``."""
