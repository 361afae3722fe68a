"""Mirror of the reference package layout (the touch chart predictor and its trainer)."""
