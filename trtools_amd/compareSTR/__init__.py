"""compareSTR: concordance of two call sets (host layer of the trk_compare device pass)."""
