"""Mirror of the reference package layout (the action samplers the DDQN learner draws from)."""
