"""Only the pre-processing defences that the reference keeps under attack/SIadv are mirrored (baselines/defense/drop_points);
the SI-Adv attack itself is out of scope."""
