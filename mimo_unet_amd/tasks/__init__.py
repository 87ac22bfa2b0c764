"""Task glue of the reference (mimo/tasks/): data modules and callbacks."""
