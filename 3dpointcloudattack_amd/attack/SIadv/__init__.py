"""Only the pre-processing defences that the reference keeps under attack/SIadv are mirrored (baselines/defense: drop_points,
DUP_Net);
the SI-Adv attack itself is out of scope."""
