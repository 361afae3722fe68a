"""Mirror of the reference package layout (the fixed-trajectory policies: ``LEBA.Engine``, ``MFBA.Engine``)."""
