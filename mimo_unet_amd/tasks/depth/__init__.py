"""The depth task (mimo/tasks/depth/): the NYUv2 data module."""
